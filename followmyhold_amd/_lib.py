"""ctypes binding of libfoho_hip.so (C ABI declared in include/foho_hip.h).

The HIP library is the product path: importing this module never falls back to a CPU
implementation -- `lib()` raises if the shared object is missing and every wrapper raises
FohoError on a non-zero status.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("FOHO_HIP_SO") or os.path.join(_HERE, "libfoho_hip.so")   # $FOHO_HIP_SO: another build of the same library (development)
_lib = None

c_f = ctypes.c_float
c_i = ctypes.c_int32
vp = ctypes.c_void_p


class FohoError(RuntimeError):
    pass


class FohoImage(ctypes.Structure):
    _fields_ = [("v_off", c_i), ("Vh", c_i), ("Vo", c_i), ("f_off", c_i), ("Fh", c_i), ("Fo", c_i),
                ("n_edges", c_i), ("jcols", c_i), ("k00", c_f), ("k11", c_f), ("cam_R", c_f * 9),
                ("cam_T", c_f * 3), ("znear", c_f), ("zfar", c_f), ("T_h2m", c_f * 12)]


class FohoDims(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("Vtot", c_i), ("Ftot", c_i), ("Vmax", c_i), ("Fmax", c_i),
                ("Vh_max", c_i), ("Vo_max", c_i), ("grid_res", c_i), ("frac_cap", c_i), ("n_renders", c_i),
                ("Fh_max", c_i), ("Fo_max", c_i), ("gbuf_f16", c_i)]


class FohoRenderCfg(ctypes.Structure):
    _fields_ = [("face_set", c_i), ("normal_mask", c_i), ("disp_mask", c_i), ("sil_mask", c_i),
                ("w_normal", c_f), ("w_disp", c_f), ("w_sil", c_f)]


class FohoStepCfg(ctypes.Structure):
    _fields_ = [("render", FohoRenderCfg * 2), ("w_kps", c_f), ("w_trans_hand", c_f), ("w_trans_obj", c_f),
                ("w_verts_obj", c_f), ("w_edge", c_f), ("w_contact", c_f), ("contact_margin", c_f),
                ("use_intersection", c_i), ("w_int_near", c_f), ("w_int_far", c_f), ("int_gate", c_f),
                ("int_gate_step_ok", c_i), ("sigma", c_f), ("gamma", c_f), ("blur_radius", c_f),
                ("lr", c_f * 16), ("beta1", c_f), ("beta2", c_f), ("eps", c_f), ("weight_decay", c_f),
                ("do_update", c_i), ("world_space_input", c_i), ("deferred_update", c_i), ("n_active_renders", c_i),
                ("listed_cap", c_i)]


class FohoStepDesc(ctypes.Structure):
    _fields_ = [("dims", FohoDims), ("images", vp), ("verts_in", vp), ("faces", vp), ("inc_off", vp),
                ("inc_fc", vp), ("nbr_off", vp), ("nbr_idx", vp), ("J_regressor", vp), ("tgt_normal", vp),
                ("tgt_disp", vp), ("mask", vp), ("kps_2d", vp), ("params", vp), ("adam_m", vp), ("adam_v", vp),
                ("adam_t", vp), ("losses", vp), ("grad_params", vp), ("grad_verts_in", vp), ("flags", vp),
                ("workspace", vp), ("workspace_bytes", ctypes.c_size_t), ("hand_order_valid", c_i),
                ("hand_faces_per_block", c_i)]


# enums of include/foho_hip.h
FACES_HAND, FACES_OBJ, FACES_ALL = 0, 1, 2
MASK_NONE, MASK_HAND, MASK_OBJ, MASK_HOI = 0, 1, 2, 3
STAGE_VERTEX, STAGE_RASTER, STAGE_LOSS, STAGE_BACKWARD, STAGE_INSIDE, STAGE_FINAL, STAGE_BBOX = 1, 2, 4, 8, 16, 32, 64
STAGE_STEP, STAGE_ALL, STAGE_TARGETS = 63, 127, 256
N_LOSS = 24
LOSS_NAMES = ["total", "intersection", "contact", "kps", "trans_hand", "trans_obj", "verts_obj", "edge", "normal0",
              "disp0", "sil0", "normal1", "disp1", "sil1", "n_intersect", "w_int", "mean_d2"]
WS_REGIONS = ["world", "ndc", "vn", "p2f", "zbuf", "sdist", "prod", "knn_idx", "knn_d2", "gworld", "frac_count",
              "stats", "parity", "frag_count", "seg_count", "hand_order"]
N_KERNELS = 10
ABI_VERSION = 105     # 105 = foho_vae_fwd / _bwd, foho_geo_weights.flags, foho_geo_gemm variant bits, FOHO_API visibility; 104 = foho_geo_weights.ln_{q,kv,2}_eps, foho_geo_decode_bwd_rows, foho_geo_prepare_queries / _decode_fwd_cached; include/foho_hip.h: 102 = foho_step_cfg.listed_cap, foho_step_desc.hand_order_valid, foho_abi_sizes; 103 = foho_geo_weights.q_norm / k_norm, foho_geo_abi_size


# ------------------------------------------------------------------------------------------------ libfoho_hip.so
# include/foho_hip.h, in its order: {function: (restype, argtypes)}.  int / int32_t -> c_i, int64_t -> c_l, size_t -> c_z,
# float -> c_f, double -> c_d, every pointer or array -> vp (POINTER of the mirror for the step structs above; the mirrors of
# geo_decode.py, sdpa.py and vae_transformer.py go in as ctypes.byref).  tests/test_cabi.py compares it with the header.
c_l, c_z, c_d = ctypes.c_int64, ctypes.c_size_t, ctypes.c_double
_DIMS, _DESC, _CFG = ctypes.POINTER(FohoDims), ctypes.POINTER(FohoStepDesc), ctypes.POINTER(FohoStepCfg)
_WS = [vp, c_z, vp]                                                 # workspace, workspace_bytes, stream
_ICP_TAIL = [c_i, c_i, c_i, c_d, c_d, vp, vp, vp] + _WS            # n_iter n_outliers fixed_scale, min_scale max_scale, T_out cost_out cost_history
_LBS_MODEL = [vp, vp, vp, vp, vp, vp, c_i]                          # v_template shapedirs posedirs J_regressor lbs_weights parents, V
_SIGNATURES = {
    "foho_last_error": (ctypes.c_char_p, []), "foho_version": (c_i, []), "foho_abi_sizes": (c_i, [vp]),
    "foho_step_workspace_bytes": (c_z, [_DIMS]), "foho_step_workspace_region": (c_l, [_DIMS, c_i, vp]),
    "foho_step_run": (c_i, [_DESC, _CFG, c_i, vp]), "foho_step_finalize": (c_i, [_DESC, _CFG, vp]),
    "foho_step_run_profiled": (c_i, [_DESC, _CFG, vp, vp]), "foho_kernel_name": (ctypes.c_char_p, [c_i]),
    # verts_ndc faces, V F H W, blur_radius sigma, pix_to_face zbuf bary dists sil_prod overflow_flag
    "foho_raster_fwd": (c_i, [vp, vp, c_i, c_i, c_i, c_i, c_f, c_f, vp, vp, vp, vp, vp, vp] + _WS),
    "foho_raster_workspace_bytes": (c_z, [c_i, c_i, c_i, c_i]),
    "foho_raster_bwd": (c_i, [vp, vp, c_i, c_i, c_i, c_i, vp, vp, vp, vp, vp, c_f, vp]),
    "foho_raster_sil_bwd": (c_i, [vp, vp, c_i, c_i, c_i, c_i, vp, vp, vp, c_f, c_f, vp]),
    "foho_knn1_fwd": (c_i, [vp, c_i, vp, c_i, vp, vp, vp]), "foho_point_mesh_dist": (c_i, [vp, vp, c_i, c_i, vp, c_i, vp, vp, vp]),
    "foho_inside_points": (c_i, [vp, vp, c_i, c_i, vp, c_i, vp, vp]), "foho_lbs_workspace_bytes": (c_z, [c_i, c_i]),
    "foho_lbs_fwd": (c_i, _LBS_MODEL + [vp, vp, c_i, c_i, vp, vp] + _WS),          # betas rot_mats, B use_mfma, verts joints
    "foho_lbs_bwd": (c_i, _LBS_MODEL + [vp, c_i, vp, vp, vp, vp] + _WS),           # rot_mats, B, grad_verts grad_joints grad_betas grad_rot_mats
    "foho_icp_workspace_bytes": (c_z, [c_i, c_i]), "foho_icp_run": (c_i, [vp, c_i, vp, c_i] + _ICP_TAIL),
    "foho_icp_batch_workspace_bytes": (c_z, [c_i, c_i, c_i]), "foho_icp_run_batch": (c_i, [vp, c_i, c_i, vp, c_i] + _ICP_TAIL),
    "foho_icp_surface_workspace_bytes": (c_z, [c_i, c_i, c_i]), "foho_icp_run_surface": (c_i, [vp, c_i, c_i, vp, c_i, vp, c_i] + _ICP_TAIL),
    "foho_flexi_workspace_bytes": (c_z, [c_i]), "foho_topology_workspace_bytes": (c_z, [c_i]), "foho_object_workspace_bytes": (c_z, [c_i, c_i]),
    "foho_flexi_fwd": (c_i, [vp, vp, c_i, vp, c_i, vp, c_i, vp, vp] + _WS),       # x s, res, verts verts_cap, faces faces_cap, l_dev counts
    "foho_flexi_bwd": (c_i, [vp, vp, c_i, vp, c_i, vp, vp] + _WS),                 # x s, res, grad_verts n_verts, grad_s grad_x
    "foho_topology_tables": (c_i, [vp, c_i, c_i, vp, vp, vp, vp, vp] + _WS),       # faces, V F, obj_flag inc_off inc_fc nbr_idx flag
    "foho_object_update": (c_i, [_DESC, vp, vp, c_i, vp] + _WS),                   # desc, counts obj_faces, faces_cap, obj_flag
    "foho_mesh_decimate": (c_i, [vp, c_i, vp, c_i, c_i, vp, vp, vp]),
    # foho_geo_*: w first; chunk_rows is c_i, n_queries / row_cap are c_l, every *_bytes is c_z
    "foho_geo_abi_size": (c_l, []), "foho_geo_workspace_bytes": (c_z, [vp, c_i]), "foho_geo_bwd_workspace_bytes": (c_z, [vp, c_i]),
    "foho_geo_saved_bytes": (c_z, [vp, c_i, c_l]), "foho_geo_query_cache_bytes": (c_z, [vp, c_l]),
    "foho_geo_rows_workspace_bytes": (c_z, [c_l, c_l, c_i]),
    "foho_geo_prepare": (c_i, [vp, vp, c_i] + _WS), "foho_geo_set_kv": (c_i, [vp, vp, c_i] + _WS),
    "foho_geo_decode_fwd": (c_i, [vp, vp, c_l, vp, c_i] + _WS),
    "foho_geo_decode_fwd_keep": (c_i, [vp, vp, c_l, vp, c_i, vp, c_z, vp, c_z] + _WS),            # .. workspace, bwd_workspace, saved
    "foho_geo_decode_bwd": (c_i, [vp, vp, c_l, vp, vp, c_i, vp, c_z, vp, c_z] + _WS),
    "foho_geo_prepare_queries": (c_i, [vp, vp, c_l, c_i, vp, c_z] + _WS),                           # .. workspace, cache
    "foho_geo_decode_fwd_cached": (c_i, [vp, vp, c_l, vp, c_z, vp, c_i] + _WS),
    "foho_geo_decode_bwd_rows": (c_i, [vp, vp, c_l, vp, vp, c_l, c_i, vp, c_z, vp, c_z, vp, c_z, vp, vp]),   # .. rows_workspace, stats_out, stream
    "foho_sdpa_workspace_bytes": (c_z, [c_i, c_i, c_i]),
    "foho_sdpa_fwd": (c_i, [vp, vp, vp, vp, vp, vp, vp] + _WS),                    # d, q k v, out nlse lse_natural
    "foho_sdpa_bwd": (c_i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp] + _WS),        # d, q k v, out nlse, grad_out grad_q grad_k grad_v
    "foho_vae_abi_size": (c_l, []), "foho_vae_workspace_bytes": (c_z, [vp]), "foho_vae_saved_bytes": (c_z, [vp]),
    "foho_vae_fwd": (c_i, [vp, vp, vp, vp, c_z] + _WS), "foho_vae_bwd": (c_i, [vp, vp, vp, vp, c_z] + _WS),    # d, x0 out | grad_out grad_x0, workspace, saved
    "foho_geo_gemm": (c_i, [vp, vp, vp, vp, vp, c_i, c_i, c_i, c_i, c_f, vp]),    # A Wt bias R C, M N K gelu, scale
    "foho_geo_attention": (c_i, [vp, vp, vp, vp, c_i, c_i, c_i, vp]), "foho_geo_last_error": (ctypes.c_char_p, [])}


def _declare(L, path, signatures):
    for fn, (restype, argtypes) in signatures.items():
        try:
            f = getattr(L, fn)
        except AttributeError:      # an older library of the same version number: additive entry points are recognised by their symbol
            raise FohoError(f"{path} does not export {fn}: rebuild (make -C followmyhold_amd/csrc)") from None
        f.restype, f.argtypes = restype, argtypes


# the side libraries: libfoho_<name>.so exports foho_<name>_* (C ABI csrc/foho_<name>.h) and is of version FOHO_<NAME>_VERSION
SIDE_VERSIONS = {"vol": 100, "sflexi": 100, "rastk": 101, "wflexi": 100, "mreg": 100}      # rastk 101 = foho_rastk_blend_fwd / _bwd
_sides = {}


def side_path(name):
    return os.path.join(_HERE, f"libfoho_{name}.so")


def build(force=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir)] + [os.path.join(_HERE, "..", "include", "foho_hip.h")]
    libs = [SO_PATH] + [side_path(n) for n in SIDE_VERSIONS]      # the same make builds them
    if force or not all(os.path.exists(p) for p in libs) or max(map(os.path.getmtime, srcs)) > min(map(os.path.getmtime, libs)):
        subprocess.check_call(["make", "-C", src_dir, "-s"])
    return SO_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise FohoError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)")
        L = ctypes.CDLL(SO_PATH)
        sizes = (ctypes.c_int64 * 5)()
        ver = L.foho_abi_sizes(sizes)
        mine = [ctypes.sizeof(t) for t in (FohoImage, FohoDims, FohoRenderCfg, FohoStepCfg, FohoStepDesc)]
        if list(sizes) != mine or ver < ABI_VERSION:
            raise FohoError(f"{SO_PATH} is ABI version {ver} with struct sizes {list(sizes)}; this binding is version "
                            f"{ABI_VERSION} with {mine}: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')")
        _declare(L, SO_PATH, _SIGNATURES)
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        raise FohoError(f"{what} failed ({status}): {lib().foho_last_error().decode()}")


def geo_error():
    """Last error of the foho_geo_* / foho_vae_* / foho_sdpa_* entry points (csrc/foho_geo.hip keeps its own string)."""
    return lib().foho_geo_last_error().decode()


def geo_check(status, what):
    if status != 0:
        raise FohoError(f"{what} failed ({status}): {geo_error()}")


def load_side(name, signatures):
    """libfoho_<name>.so with `signatures` ({function: (restype, argtypes)}) set.  No CPU path: raises when the library is missing or
    of another version."""
    L = _sides.get(name)
    if L is None:
        path, version = side_path(name), SIDE_VERSIONS[name]
        if not os.path.exists(path):
            raise FohoError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
        L = ctypes.CDLL(path)
        ver = getattr(L, f"foho_{name}_version")
        ver.restype = ctypes.c_int
        if ver() != version:
            raise FohoError(f"{path} is version {ver()}, this binding is {version}: rebuild (make -C followmyhold_amd/csrc)")
        getattr(L, f"foho_{name}_last_error").restype = ctypes.c_char_p
        _declare(L, path, signatures)
        _sides[name] = L
    return L


def check_side(lib, prefix, status, what):
    if status != 0:
        raise FohoError(f"{what} failed ({status}): {getattr(lib, prefix + '_last_error')().decode()}")


def _p(t):      # a tensor's address, or None (NULL): the declared argtypes take the plain integer, no ctypes object per argument
    return None if t is None else t.data_ptr()


def _stream(device):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


# ------------------------------------------------------------------------------------------------ libfoho_rastk.so
RASTK_SO_PATH = side_path("rastk")
RASTK_VERSION = SIDE_VERSIONS["rastk"]      # FOHO_RASTK_VERSION of csrc/foho_rastk.h
RASTK_MAX_K = 128        # FOHO_RASTK_MAX_K
RASTK_CULL_BACKFACES, RASTK_OVER_LIST = 1, 1
RASTK_BLEND_MAX_D = 4    # FOHO_RASTK_BLEND_MAX_D
RASTK_BLEND_UNIT_BARY, RASTK_BLEND_ALPHA_ONLY = 1, 2
_RASTK_BLEND_HEAD = [vp, vp, vp, vp, vp, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, vp, c_i]     # planes, face_attr, F H W K D, sigma gamma znear zfar, background, flags
# verts_ndc, faces, V F H W K, blur_radius, raster_flags, face_attr, D, sigma gamma znear zfar, background, blend_flags
_RASTK_RENDER_HEAD = [vp, vp, c_i, c_i, c_i, c_i, c_i, c_f, c_i, vp, c_i, c_f, c_f, c_f, c_f, vp, c_i]
_RASTK_SIGNATURES = {
    "foho_rastk_blend_fwd": (ctypes.c_int, _RASTK_BLEND_HEAD + [vp, vp]),
    "foho_rastk_blend_bwd": (ctypes.c_int, _RASTK_BLEND_HEAD + [vp, vp, vp, vp, vp, vp]),
    "foho_rastk_workspace_bytes": (ctypes.c_size_t, [c_i, c_i, c_i, c_i, c_i, ctypes.c_int64]),
    "foho_rastk_fwd": (ctypes.c_int, [vp, vp, c_i, c_i, c_i, c_i, c_i, c_f, c_i, vp, vp, vp, vp, vp, vp, ctypes.c_int64, vp, ctypes.c_size_t, vp]),
    "foho_rastk_bwd": (ctypes.c_int, [vp, vp, c_i, c_i, c_i, c_i, c_i, vp, vp, vp, vp, vp, c_f, vp]),
    # foho_rastk_render_*: _RASTK_RENDER_HEAD, then out, counts, overflow | grad_out, grad_verts_ndc, grad_face_attr, then list_cap, workspace, bytes, stream
    "foho_rastk_render_fwd": (ctypes.c_int, _RASTK_RENDER_HEAD + [vp, vp, vp, ctypes.c_int64, vp, ctypes.c_size_t, vp]),
    "foho_rastk_render_bwd": (ctypes.c_int, _RASTK_RENDER_HEAD + [vp, vp, vp, ctypes.c_int64, vp, ctypes.c_size_t, vp])}


def rastk():
    """libfoho_rastk.so (C ABI csrc/foho_rastk.h): the K-fragment rasteriser."""
    return load_side("rastk", _RASTK_SIGNATURES)


def rastk_check(status, what):
    check_side(rastk(), "foho_rastk", status, what)
