"""Python wrappers of the stand-alone C-ABI operators (torch tensors in, torch tensors out; no CPU fallback).

Each function states the reference interface it replaces.  All launches go to the current torch stream.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from ._lib import _p, _stream
from .sparse_flexi import flexicubes_sparse, flexicubes_sparse_grad, grid_axes  # noqa: F401  (the extractors on axis tables: sparse_flexi.py)
from .weighted_flexi import flexicubes_weighted  # noqa: F401  (alpha, beta, gamma, training mode, all gradients: weighted_flexi.py)
from .mesh_reg import MeshTopology, mesh_regularizers  # noqa: F401  (Laplacian, normal consistency, edge length, fused, with gradient: mesh_reg.py)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.FohoError("libfoho_hip operators need CUDA/HIP tensors (there is no CPU fallback)")


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------ rasteriser
def raster_fwd(verts_ndc, faces, H, W, blur_radius, sigma=1e-8, want_sil=True):
    """pytorch3d rasterize_meshes(K=1) (+ the K=100 silhouette product) for one mesh.
    Returns dict(pix_to_face (H,W) int64, zbuf, bary (H,W,3), dists, sil_prod (H,W) or None)."""
    _need_cuda(verts_ndc, faces)
    lib = L.lib()
    v, f = _f32(verts_ndc), faces.detach().to(torch.int32).contiguous()
    V, F = v.shape[0], f.shape[0]
    dev = v.device
    nws = lib.foho_raster_workspace_bytes(V, F, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    p2f = torch.empty(H, W, dtype=torch.int64, device=dev)
    zb, di = torch.empty(H, W, device=dev), torch.empty(H, W, device=dev)
    ba = torch.empty(H, W, 3, device=dev)
    pr = torch.empty(H, W, device=dev) if want_sil else None
    ov = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.foho_raster_fwd(_p(v), _p(f), V, F, H, W, blur_radius, sigma, _p(p2f), _p(zb), _p(ba), _p(di), _p(pr), _p(ov),
                                _p(ws), nws, _stream(dev)), "foho_raster_fwd")
    return dict(pix_to_face=p2f, zbuf=zb, bary=ba, dists=di, sil_prod=pr, overflow=ov, _keep=(v, f, ws))


def raster_bwd(verts_ndc, faces, pix_to_face, grad_zbuf=None, grad_bary=None, grad_dists=None, blur_radius=0.0):
    """Backward of the K=1 fragments -> grad w.r.t. verts_ndc (V,3).  blur_radius: the forward call's."""
    lib = L.lib()
    v, f = _f32(verts_ndc), faces.detach().to(torch.int32).contiguous()
    H, W = pix_to_face.shape[-2:]
    g = torch.zeros_like(v)
    gz = _f32(grad_zbuf) if grad_zbuf is not None else None
    gb = _f32(grad_bary) if grad_bary is not None else None
    gd = _f32(grad_dists) if grad_dists is not None else None
    p2f = pix_to_face.contiguous()
    L.check(lib.foho_raster_bwd(_p(v), _p(f), v.shape[0], f.shape[0], H, W, _p(p2f), _p(gz), _p(gb), _p(gd), _p(g), blur_radius,
                                _stream(v.device)), "foho_raster_bwd")
    return g


def raster_sil_bwd(verts_ndc, faces, sil_prod, grad_prod, blur_radius, sigma):
    """Backward of the silhouette product of raster_fwd -> grad w.r.t. verts_ndc (V,3)."""
    lib = L.lib()
    v, f = _f32(verts_ndc), faces.detach().to(torch.int32).contiguous()
    H, W = sil_prod.shape[-2:]
    g = torch.zeros_like(v)
    pr, gp = _f32(sil_prod), _f32(grad_prod)
    L.check(lib.foho_raster_sil_bwd(_p(v), _p(f), v.shape[0], f.shape[0], H, W, _p(pr), _p(gp), _p(g), blur_radius, sigma,
                                    _stream(v.device)), "foho_raster_sil_bwd")
    return g


# ------------------------------------------------------------------------------------------------ K-fragment rasteriser
def _raster_k_shapes(verts_ndc, faces, H, W, K, who="raster_k"):
    """The shape, dtype and range checks of the K-fragment operators (no device is asked for)."""
    K, H, W = int(K), int(H), int(W)
    if K < 1 or K > L.RASTK_MAX_K:
        raise ValueError(f"{who}: K = {K} outside 1 .. {L.RASTK_MAX_K} (not clamped)")
    if H < 1 or W < 1 or H > 8192 or W > 8192 or H * W > (1 << 25):
        raise ValueError(f"{who}: frame {H} x {W} out of range")
    if verts_ndc.dim() != 2 or verts_ndc.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or not len(verts_ndc) or not len(faces):
        raise ValueError(f"{who}: expected (V,3) vertices and (F,3) faces")
    if faces.dtype not in (torch.int32, torch.int64) or not faces.is_contiguous():
        raise ValueError(f"{who}: faces must be a contiguous int32 or int64 tensor")
    return K, H, W


def _raster_k_args(verts_ndc, faces, H, W, K):
    """Argument checks of raster_k_fwd / raster_k_bwd, before any device work."""
    K, H, W = _raster_k_shapes(verts_ndc, faces, H, W, K)
    _need_cuda(verts_ndc, faces)
    return K, H, W


def _with_tile_lists(who, shape, cap, ov, launch):
    """launch(cap, workspace) of raster_k_fwd / render_k_fwd (`who`) with a workspace whose per-tile face lists hold `cap` entries, and,
    when the overflow word `ov` says afterwards that they were too short, once more at the size the first pass left in the workspace.
    Returns (workspace, cap, retried)."""
    V, F, H, W, K = shape
    retried = False
    while True:
        nws = L.rastk().foho_rastk_workspace_bytes(V, F, H, W, K, cap)
        if nws == 0:
            raise L.FohoError(f"{who}: no workspace size for V={V} F={F} H={H} W={W} K={K} list_cap={cap}")
        ws = torch.empty(nws, dtype=torch.uint8, device=ov.device)
        launch(cap, ws)
        if not (int(ov.item()) & L.RASTK_OVER_LIST):      # one host read per call: the list size is data dependent
            return ws, cap, retried
        if retried:
            raise L.FohoError(f"{who}: the tile lists overflowed again at the size the first pass reported")
        cap, retried = int(ws[:8].view(torch.int64).item()), True


def raster_k_fwd(verts_ndc, faces, H, W, K, blur_radius, cull_backfaces=False, list_cap=None):
    """pytorch3d rasterize_meshes(faces_per_pixel=K) for one mesh, materialised (libfoho_rastk.so; 1 <= K <= 128).
    Returns dict(pix_to_face (H,W,K) int64, zbuf (H,W,K), bary (H,W,K,3), dists (H,W,K), counts (H,W) int32 [fragments the pixel
    received before the cut at K]); background entries are -1.  list_cap: capacity of the per-tile face lists in entries; when
    the scene needs more, the call is repeated once with the exact size (`retried` in the result says so)."""
    K, H, W = _raster_k_args(verts_ndc, faces, H, W, K)
    lib = L.rastk()
    v, f = _f32(verts_ndc), faces.detach().to(torch.int32)
    V, F = v.shape[0], f.shape[0]
    dev = v.device
    cap = int(list_cap) if list_cap is not None else max(4 * F, 1024)
    p2f = torch.empty(H, W, K, dtype=torch.int64, device=dev)
    zb, di = torch.empty(H, W, K, device=dev), torch.empty(H, W, K, device=dev)
    ba = torch.empty(H, W, K, 3, device=dev)
    cn = torch.empty(H, W, dtype=torch.int32, device=dev)
    ov = torch.zeros(1, dtype=torch.int32, device=dev)
    flags = L.RASTK_CULL_BACKFACES if cull_backfaces else 0

    def launch(cap, ws):
        L.rastk_check(lib.foho_rastk_fwd(_p(v), _p(f), V, F, H, W, K, float(blur_radius), flags, _p(p2f), _p(zb), _p(ba), _p(di), _p(cn),
                                         _p(ov), cap, _p(ws), ws.numel(), _stream(dev)), "foho_rastk_fwd")
    ws, cap, retried = _with_tile_lists("raster_k_fwd", (V, F, H, W, K), cap, ov, launch)
    return dict(pix_to_face=p2f, zbuf=zb, bary=ba, dists=di, counts=cn, retried=retried, list_cap=cap, workspace_bytes=ws.numel())


def raster_k_bwd(verts_ndc, faces, pix_to_face, grad_zbuf=None, grad_bary=None, grad_dists=None, blur_radius=0.0):
    """Backward of all H W K fragments of raster_k_fwd -> grad w.r.t. verts_ndc (V,3).  pix_to_face: (H,W,K); any of the three
    gradients may be None.  blur_radius: the forward call's."""
    if pix_to_face.dim() != 3 or pix_to_face.dtype != torch.int64:
        raise ValueError("raster_k_bwd: pix_to_face must be (H,W,K) int64")
    H, W, K = pix_to_face.shape
    _raster_k_args(verts_ndc, faces, H, W, K)
    lib = L.rastk()
    v, f = _f32(verts_ndc), faces.detach().to(torch.int32)
    g = torch.zeros_like(v)
    gz = _f32(grad_zbuf) if grad_zbuf is not None else None
    gb = _f32(grad_bary) if grad_bary is not None else None
    gd = _f32(grad_dists) if grad_dists is not None else None
    for t, shape in ((gz, (H, W, K)), (gb, (H, W, K, 3)), (gd, (H, W, K))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"raster_k_bwd: gradient of shape {tuple(t.shape)}, expected {shape}")
    p2f = pix_to_face.contiguous()
    L.rastk_check(lib.foho_rastk_bwd(_p(v), _p(f), v.shape[0], f.shape[0], H, W, K, _p(p2f), _p(gz), _p(gb), _p(gd), _p(g), float(blur_radius),
                                     _stream(v.device)), "foho_rastk_bwd")
    return g


class _RasterKFn(torch.autograd.Function):
    """raster_k_fwd / raster_k_bwd as one differentiable operator (w.r.t. verts_ndc)."""

    @staticmethod
    def forward(ctx, verts_ndc, faces, H, W, K, blur_radius, cull_backfaces):
        out = raster_k_fwd(verts_ndc, faces, H, W, K, blur_radius, cull_backfaces)
        ctx.blur = float(blur_radius)
        ctx.save_for_backward(verts_ndc.detach(), faces, out["pix_to_face"])
        ctx.mark_non_differentiable(out["pix_to_face"], out["counts"])
        return out["pix_to_face"], out["zbuf"], out["bary"], out["dists"], out["counts"]

    @staticmethod
    def backward(ctx, _gp, g_z, g_b, g_d, _gc):
        v, f, p2f = ctx.saved_tensors
        g = raster_k_bwd(v, f, p2f, g_z, g_b, g_d, blur_radius=ctx.blur)
        return g.to(v.dtype), None, None, None, None, None, None


def raster_k(verts_ndc, faces, H, W, K, blur_radius, cull_backfaces=False):
    """(pix_to_face, zbuf, bary, dists, counts) of raster_k_fwd, differentiable w.r.t. verts_ndc."""
    return _RasterKFn.apply(verts_ndc, faces, int(H), int(W), int(K), float(blur_radius), bool(cull_backfaces))


# ------------------------------------------------------------------------------------------------ shading + blend of K-fragment planes
def _blend_k_scalars(face_attr, sigma, gamma, znear, zfar, background, alpha_only, who="blend_k"):
    """The checks of the blend's scalars, attributes and background (no device is asked for).  Returns (D, F, background array)."""
    if not float(sigma) > 0.0:
        raise ValueError(f"{who}: sigma must be positive")
    D, F, bg = 1, 1, None
    if not alpha_only:
        if face_attr is None or face_attr.dim() != 3 or face_attr.shape[1] != 3 or face_attr.dtype != torch.float32 or not len(face_attr):
            raise ValueError(f"{who}: face_attr must be a float32 tensor of shape (F,3,D)")
        F, _, D = face_attr.shape
        if D < 1 or D > L.RASTK_BLEND_MAX_D:
            raise ValueError(f"{who}: D = {D} outside 1 .. {L.RASTK_BLEND_MAX_D}")
        if not float(gamma) > 0.0 or not float(zfar) > float(znear):
            raise ValueError(f"{who}: gamma must be positive and zfar above znear")
        bg = [float(x) for x in (background.tolist() if torch.is_tensor(background) else background)]
        if len(bg) != D:
            raise ValueError(f"{who}: background has {len(bg)} entries, the face attributes {D} channels")
        bg = (ctypes.c_float * D)(*bg)
    return D, F, bg


def _blend_k_args(pix_to_face, zbuf, bary, dists, face_attr, sigma, gamma, znear, zfar, background, unit_bary, alpha_only, grad_out=None):
    """Argument checks of blend_k_fwd / blend_k_bwd, before any device work.  Returns (H, W, K, D, F, flags, background array)."""
    if pix_to_face.dim() != 3 or pix_to_face.dtype != torch.int64:
        raise ValueError("blend_k: pix_to_face must be (H,W,K) int64")
    H, W, K = pix_to_face.shape
    if K < 1 or K > L.RASTK_MAX_K:
        raise ValueError(f"blend_k: K = {K} outside 1 .. {L.RASTK_MAX_K} (not clamped)")
    if H < 1 or W < 1 or H > 8192 or W > 8192 or H * W > (1 << 25):
        raise ValueError(f"blend_k: frame {H} x {W} out of range")
    planes = [("dists", dists, (H, W, K))]
    if not alpha_only:
        planes.append(("zbuf", zbuf, (H, W, K)))
        if not unit_bary:
            planes.append(("bary", bary, (H, W, K, 3)))
    for name, t, shape in planes:
        if t is None or tuple(t.shape) != shape or t.dtype != torch.float32:
            raise ValueError(f"blend_k: {name} must be a float32 tensor of shape {shape}")
    D, F, bg = _blend_k_scalars(face_attr, sigma, gamma, znear, zfar, background, alpha_only)
    if grad_out is not None and tuple(grad_out.shape) != ((H, W) if alpha_only else (H, W, D + 1)):
        raise ValueError(f"blend_k_bwd: grad_out of shape {tuple(grad_out.shape)}")
    _need_cuda(grad_out, pix_to_face, dists, None if alpha_only else zbuf, None if alpha_only or unit_bary else bary, None if alpha_only else face_attr)
    flags = (L.RASTK_BLEND_UNIT_BARY if unit_bary else 0) | (L.RASTK_BLEND_ALPHA_ONLY if alpha_only else 0)
    return H, W, K, D, F, flags, bg


def _blend_k_head(pix_to_face, zbuf, bary, dists, face_attr, sigma, gamma, znear, zfar, background, unit_bary, alpha_only, grad_out=None):
    """The checked arguments both entry points of the library share (its C order) and the tensors they point into."""
    H, W, K, D, F, flags, bg = _blend_k_args(pix_to_face, zbuf, bary, dists, face_attr, sigma, gamma, znear, zfar, background, unit_bary,
                                             alpha_only, grad_out)
    keep = [pix_to_face.contiguous(), None if alpha_only else zbuf.detach().contiguous(),
            None if alpha_only or unit_bary else bary.detach().contiguous(), dists.detach().contiguous(),
            None if alpha_only else face_attr.detach().contiguous()]
    head = [_p(t) for t in keep] + [F, H, W, K, D, float(sigma), float(gamma), float(znear), float(zfar), bg, flags]
    return (H, W, K, D, F), head, keep


def blend_k_fwd(pix_to_face, zbuf, bary, dists, face_attr, sigma, gamma, znear, zfar, background, unit_bary=False, alpha_only=False):
    """facade.interpolate_face_attributes + softmax_rgb_blend over the (H,W,K) planes of raster_k_fwd in one launch (libfoho_rastk.so).
    face_attr (F,3,D) float32, 1 <= D <= 4; background: D floats.  Returns (H,W,D+1): the D blended channels, then the alpha
    1 - prod_k(1 - sigmoid(-dists_k / sigma)).  unit_bary: weights (1, 1, 1) in place of the barycentrics (bary may be None).
    alpha_only: (H,W) alpha from pix_to_face and dists alone (every other tensor may be None).
    The planes are front-packed, as raster_k_fwd writes them: everything from a pixel's first negative id on is ignored."""
    (H, W, K, D, F), head, keep = _blend_k_head(pix_to_face, zbuf, bary, dists, face_attr, sigma, gamma, znear, zfar, background, unit_bary,
                                                alpha_only)
    out = torch.empty((H, W) if alpha_only else (H, W, D + 1), device=dists.device)
    L.rastk_check(L.rastk().foho_rastk_blend_fwd(*head, _p(out), _stream(dists.device)), "foho_rastk_blend_fwd")
    return out


def blend_k_bwd(pix_to_face, zbuf, bary, dists, face_attr, sigma, gamma, znear, zfar, background, grad_out, unit_bary=False,
                alpha_only=False, need=(True, True, True, True)):
    """Backward of blend_k_fwd: (grad_zbuf, grad_bary, grad_dists, grad_face_attr), None where `need` is False (the library is
    handed a null pointer and skips that output) and where the mode has no such input (unit_bary: bary; alpha_only: all but dists)."""
    (H, W, K, D, F), head, keep = _blend_k_head(pix_to_face, zbuf, bary, dists, face_attr, sigma, gamma, znear, zfar, background, unit_bary,
                                                alpha_only, grad_out)
    go = _f32(grad_out)
    dev = dists.device
    need = [bool(n) for n in need]
    if alpha_only:
        need[0] = need[1] = need[3] = False
    if unit_bary:
        need[1] = False
    # the plane gradients are written at the pixels' fragments only: zeroed buffers
    shapes = ((H, W, K), (H, W, K, 3), (H, W, K), (F, 3, D))
    grads = [torch.zeros(s, device=dev) if n else None for s, n in zip(shapes, need)]
    L.rastk_check(L.rastk().foho_rastk_blend_bwd(*head, _p(go), *[_p(g) for g in grads], _stream(dists.device)), "foho_rastk_blend_bwd")
    return tuple(grads)


class _BlendKFn(torch.autograd.Function):
    """blend_k_fwd / blend_k_bwd as one differentiable operator (w.r.t. zbuf, bary, dists and face_attr)."""

    @staticmethod
    def forward(ctx, pix_to_face, zbuf, bary, dists, face_attr, cfg):
        ctx.cfg = cfg
        ctx.save_for_backward(pix_to_face, zbuf, bary, dists, face_attr)
        return blend_k_fwd(pix_to_face, zbuf, bary, dists, face_attr, *cfg)

    @staticmethod
    def backward(ctx, g_out):
        g = blend_k_bwd(*ctx.saved_tensors, *ctx.cfg[:5], g_out, *ctx.cfg[5:], need=ctx.needs_input_grad[1:5])
        return (None,) + g + (None,)


def blend_k(pix_to_face, zbuf, bary, dists, face_attr, sigma, gamma, znear, zfar, background, unit_bary=False):
    """blend_k_fwd, differentiable w.r.t. zbuf, bary, dists and face_attr; the backward computes only the gradients autograd asks for.
    Chained behind raster_k the gradient reaches the vertices through raster_k_bwd."""
    bg = tuple(float(x) for x in (background.tolist() if torch.is_tensor(background) else background))
    cfg = (float(sigma), float(gamma), float(znear), float(zfar), bg, bool(unit_bary), False)
    return _BlendKFn.apply(pix_to_face, zbuf, None if unit_bary else bary, dists, face_attr, cfg)


def blend_k_alpha(pix_to_face, dists, sigma):
    """(H,W) alpha = 1 - prod_k(1 - sigmoid(-dists_k / sigma)) over the pixel's fragments (SoftSilhouetteShader on K-fragment planes),
    differentiable w.r.t. dists.  Bitwise the last channel of blend_k."""
    cfg = (float(sigma), 1.0, 0.0, 1.0, None, False, True)
    return _BlendKFn.apply(pix_to_face, None, None, dists, None, cfg)


# ------------------------------------------------------------------------------------------------ fused K-fragment render (no planes)
def _render_k_head(verts_ndc, faces, H, W, K, blur_radius, face_attr, sigma, gamma, znear, zfar, background, cull_backfaces, unit_bary,
                   alpha_only, grad_out=None):
    """Argument checks of render_k_fwd / render_k_bwd, before any device work (ValueError for shapes, dtypes and ranges, then FohoError
    for CPU tensors), and the checked arguments both entry points of the library share (its C order) with the tensors they point into."""
    K, H, W = _raster_k_shapes(verts_ndc, faces, H, W, K, "render_k")
    if not float(blur_radius) >= 0.0:
        raise ValueError("render_k: negative blur radius")
    D, Fa, bg = _blend_k_scalars(face_attr, sigma, gamma, znear, zfar, background, alpha_only, "render_k")
    if not alpha_only and Fa != len(faces):
        raise ValueError(f"render_k: face_attr holds {Fa} faces, the mesh {len(faces)}")
    if grad_out is not None and (tuple(grad_out.shape) != ((H, W) if alpha_only else (H, W, D + 1))):
        raise ValueError(f"render_k_bwd: grad_out of shape {tuple(grad_out.shape)}")
    _need_cuda(verts_ndc, faces, None if alpha_only else face_attr, grad_out)
    keep = [_f32(verts_ndc), faces.detach().to(torch.int32), None if alpha_only else face_attr.detach().contiguous()]
    V, F = keep[0].shape[0], keep[1].shape[0]
    rflags = L.RASTK_CULL_BACKFACES if cull_backfaces else 0
    bflags = (L.RASTK_BLEND_UNIT_BARY if unit_bary else 0) | (L.RASTK_BLEND_ALPHA_ONLY if alpha_only else 0)
    head = [_p(keep[0]), _p(keep[1]), V, F, H, W, K, float(blur_radius), rflags, _p(keep[2]), D, float(sigma), float(gamma),
            float(znear), float(zfar), bg, bflags]
    return (V, F, H, W, K, D), head, keep


def render_k_fwd(verts_ndc, faces, H, W, K, blur_radius, face_attr, sigma, gamma, znear, zfar, background, cull_backfaces=False,
                 unit_bary=False, alpha_only=False, list_cap=None):
    """raster_k_fwd and blend_k_fwd in one (libfoho_rastk.so, foho_rastk_render_fwd): the K nearest fragments of every pixel are blended
    where the rasteriser selects them, and the (H,W,K) planes never exist in memory.  Returns dict(out (H,W,D+1) [or (H,W) alpha with
    alpha_only] -- bitwise blend_k_fwd on raster_k_fwd's planes --, counts (H,W) int32, workspace [the tile lists, which render_k_bwd
    reads], list_cap, retried).  list_cap: as raster_k_fwd's -- one host read of the overflow word per call, and one repeat at the
    exact size when the scene needs more."""
    (V, F, H, W, K, D), head, keep = _render_k_head(verts_ndc, faces, H, W, K, blur_radius, face_attr, sigma, gamma, znear, zfar, background,
                                                    cull_backfaces, unit_bary, alpha_only)
    lib = L.rastk()
    dev = keep[0].device
    cap = int(list_cap) if list_cap is not None else max(4 * F, 1024)
    out = torch.empty((H, W) if alpha_only else (H, W, D + 1), device=dev)
    cn = torch.empty(H, W, dtype=torch.int32, device=dev)
    ov = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch(cap, ws):
        L.rastk_check(lib.foho_rastk_render_fwd(*head, _p(out), _p(cn), _p(ov), cap, _p(ws), ws.numel(), _stream(dev)), "foho_rastk_render_fwd")
    ws, cap, retried = _with_tile_lists("render_k_fwd", (V, F, H, W, K), cap, ov, launch)
    return dict(out=out, counts=cn, workspace=ws, list_cap=cap, retried=retried)


def render_k_bwd(verts_ndc, faces, H, W, K, blur_radius, face_attr, sigma, gamma, znear, zfar, background, grad_out, workspace, list_cap,
                 cull_backfaces=False, unit_bary=False, alpha_only=False, need=(True, True)):
    """Backward of render_k_fwd over the workspace it returned (with its list_cap): (grad_verts_ndc (V,3), grad_face_attr (F,3,D)), None
    where `need` is False (the library is handed a null pointer and skips that work) and, with alpha_only, for the attributes."""
    (V, F, H, W, K, D), head, keep = _render_k_head(verts_ndc, faces, H, W, K, blur_radius, face_attr, sigma, gamma, znear, zfar, background,
                                                    cull_backfaces, unit_bary, alpha_only, grad_out)
    lib = L.rastk()
    if workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
        raise ValueError("render_k_bwd: workspace must be the uint8 tensor render_k_fwd returned")
    _need_cuda(workspace)
    need_bytes = lib.foho_rastk_workspace_bytes(V, F, H, W, K, int(list_cap))
    if need_bytes == 0 or workspace.numel() < need_bytes:
        raise ValueError(f"render_k_bwd: workspace of {workspace.numel()} bytes, list_cap {int(list_cap)} needs {need_bytes}")
    go = _f32(grad_out)
    dev = go.device
    gv = torch.zeros(V, 3, device=dev) if need[0] else None
    ga = torch.zeros(F, 3, D, device=dev) if need[1] and not alpha_only else None
    if gv is not None or ga is not None:
        L.rastk_check(lib.foho_rastk_render_bwd(*head, _p(go), _p(gv), _p(ga), int(list_cap), _p(workspace), workspace.numel(), _stream(dev)),
                      "foho_rastk_render_bwd")
    return gv, ga


class _RenderKFn(torch.autograd.Function):
    """render_k_fwd / render_k_bwd as one differentiable operator (w.r.t. verts_ndc and face_attr); the workspace is kept for the backward."""

    @staticmethod
    def forward(ctx, verts_ndc, faces, face_attr, geom, cfg):
        r = render_k_fwd(verts_ndc, faces, *geom, face_attr, *cfg)
        ctx.geom, ctx.cfg, ctx.list_cap = geom, cfg, r["list_cap"]
        ctx.save_for_backward(verts_ndc.detach(), faces, None if face_attr is None else face_attr.detach(), r["workspace"])
        ctx.mark_non_differentiable(r["counts"])
        return r["out"], r["counts"]

    @staticmethod
    def backward(ctx, g_out, _gc):
        v, f, a, ws = ctx.saved_tensors
        gv, ga = render_k_bwd(v, f, *ctx.geom, a, *ctx.cfg[:5], g_out, ws, ctx.list_cap, *ctx.cfg[5:],
                              need=(ctx.needs_input_grad[0], ctx.needs_input_grad[2]))
        return (None if gv is None else gv.to(v.dtype)), None, ga, None, None


def render_k(verts_ndc, faces, H, W, K, blur_radius, face_attr, sigma, gamma, znear, zfar, background, cull_backfaces=False, unit_bary=False,
             return_counts=False):
    """render_k_fwd's image (H,W,D+1), differentiable w.r.t. verts_ndc and face_attr: raster_k -> blend_k as one operator whose memory does
    not grow with K.  The backward computes only the gradients autograd asks for.  Like raster_k it reads one word back per call and so
    cannot be captured in a graph.  return_counts: also the (H,W) int32 fragment counts before the cut."""
    bg = tuple(float(x) for x in (background.tolist() if torch.is_tensor(background) else background))
    cfg = (float(sigma), float(gamma), float(znear), float(zfar), bg, bool(cull_backfaces), bool(unit_bary), False)
    out, counts = _RenderKFn.apply(verts_ndc, faces, face_attr, (int(H), int(W), int(K), float(blur_radius)), cfg)
    return (out, counts) if return_counts else out


def render_k_alpha(verts_ndc, faces, H, W, K, blur_radius, sigma, cull_backfaces=False):
    """(H,W) alpha = 1 - prod_k(1 - sigmoid(-dists_k / sigma)) over the K nearest fragments, mesh to silhouette in one operator,
    differentiable w.r.t. verts_ndc.  Bitwise blend_k_alpha on raster_k's planes."""
    cfg = (float(sigma), 1.0, 0.0, 1.0, None, bool(cull_backfaces), False, True)
    return _RenderKFn.apply(verts_ndc, faces, None, (int(H), int(W), int(K), float(blur_radius)), cfg)[0]


# ------------------------------------------------------------------------------------------------ knn / sdf
def knn1(p1, p2):
    """pytorch3d.ops.knn_points(K=1): (squared distances (N1,), indices (N1,) int64)."""
    _need_cuda(p1, p2)
    lib = L.lib()
    a, b = _f32(p1), _f32(p2)
    d2 = torch.empty(a.shape[0], device=a.device)
    idx = torch.empty(a.shape[0], dtype=torch.int64, device=a.device)
    L.check(lib.foho_knn1_fwd(_p(a), a.shape[0], _p(b), b.shape[0], _p(d2), _p(idx), _stream(a.device)), "foho_knn1_fwd")
    return d2, idx


def point_mesh_dist(verts, faces, pts):
    """kaolin point_to_mesh_distance: (squared distance (N,), closest face (N,) int64)."""
    _need_cuda(verts, faces, pts)
    lib = L.lib()
    v, f, p = _f32(verts), faces.detach().to(torch.int32).contiguous(), _f32(pts)
    d2 = torch.empty(p.shape[0], device=p.device)
    fi = torch.empty(p.shape[0], dtype=torch.int64, device=p.device)
    L.check(lib.foho_point_mesh_dist(_p(v), _p(f), v.shape[0], f.shape[0], _p(p), p.shape[0], _p(d2), _p(fi), _stream(v.device)),
            "foho_point_mesh_dist")
    return d2, fi


def inside_points(verts, faces, pts):
    """kaolin check_sign: bool (N,) -- True inside the closed mesh."""
    _need_cuda(verts, faces, pts)
    lib = L.lib()
    v, f, p = _f32(verts), faces.detach().to(torch.int32).contiguous(), _f32(pts)
    out = torch.empty(p.shape[0], dtype=torch.uint8, device=p.device)
    L.check(lib.foho_inside_points(_p(v), _p(f), v.shape[0], f.shape[0], _p(p), p.shape[0], _p(out), _stream(v.device)), "foho_inside_points")
    return out.bool()


# ------------------------------------------------------------------------------------------------ LBS
class LbsModel:
    """Device copy of a MANO-shaped model (synthetic.mano_like_model() or the real MANO arrays)."""

    def __init__(self, model, device="cuda"):
        # k_lbs_joints walks the joints in index order and reads G[parents[i]]: a parent has to come before its child
        parents = [int(p) for p in np.asarray(model["parents"]).reshape(-1)]
        if len(parents) != 16 or parents[0] >= 0 or any(not 0 <= parents[i] < i for i in range(1, 16)):
            raise L.FohoError(f"LbsModel: parents must be 16 entries with parents[0] < 0 and 0 <= parents[i] < i, got {parents}")
        t = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a)).to(dt).contiguous().to(device)
        self.v_template = t(model["v_template"])
        self.shapedirs = t(model["shapedirs"])
        self.posedirs = t(model["posedirs"])
        self.J_regressor = t(model["J_regressor"])
        self.lbs_weights = t(model["lbs_weights"])
        self.parents = t(model["parents"], torch.int32)
        self.V = self.v_template.shape[0]
        assert self.shapedirs.shape == (self.V, 3, 10) and self.posedirs.shape == (135, 3 * self.V)
        assert self.J_regressor.shape == (16, self.V) and self.lbs_weights.shape == (self.V, 16)

    def _args(self):
        return [_p(x) for x in (self.v_template, self.shapedirs, self.posedirs, self.J_regressor,
                                          self.lbs_weights, self.parents)] + [self.V]


class _LbsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, betas, rot, model, use_mfma):
        lib = L.lib()
        B = betas.shape[0]
        b, r = _f32(betas), _f32(rot).reshape(B, 16, 3, 3)
        nws = lib.foho_lbs_workspace_bytes(B, model.V)
        ws = torch.empty(nws, dtype=torch.uint8, device=b.device)
        verts = torch.empty(B, model.V, 3, device=b.device)
        joints = torch.empty(B, 16, 3, device=b.device)
        L.check(lib.foho_lbs_fwd(*model._args(), _p(b), _p(r), B, int(use_mfma), _p(verts), _p(joints), _p(ws), nws, _stream(b.device)),
                "foho_lbs_fwd")
        ctx.model, ctx.ws, ctx.nws, ctx.B = model, ws, nws, B
        ctx.save_for_backward(r)
        return verts, joints

    @staticmethod
    def backward(ctx, g_verts, g_joints):
        lib = L.lib()
        (r,) = ctx.saved_tensors
        B, model = ctx.B, ctx.model
        gv = _f32(g_verts) if g_verts is not None else torch.zeros(B, model.V, 3, device=r.device)
        gj = _f32(g_joints) if g_joints is not None else None
        gb = torch.empty(B, 10, device=r.device)
        gr = torch.empty(B, 16, 3, 3, device=r.device)
        L.check(lib.foho_lbs_bwd(*model._args(), _p(r), B, _p(gv), _p(gj), _p(gb), _p(gr), _p(ctx.ws), ctx.nws, _stream(r.device)),
                "foho_lbs_bwd")
        return gb, gr, None, None


def lbs(betas, rot_mats, model: LbsModel, use_mfma=-1):
    """smplx MANOLayer(pose2rot=False): betas (B,10), rot_mats (B,16,3,3) -> verts (B,V,3), posed joints (B,16,3).
    Differentiable w.r.t. betas and rot_mats (hand-derived backward kernels)."""
    _need_cuda(betas, rot_mats)
    return _LbsFn.apply(betas, rot_mats, model, use_mfma)


# ------------------------------------------------------------------------------------------------ ICP
def icp_points_multi(start_points, target_points, n_iter, n_outliers=0, fixed_scale=False, min_scale=0.5, max_scale=2.0,
                     device="cuda", return_history=False, target_faces=None):
    """The icp() loop of src/foho/alignment/mesh_align.py:91-142 for ALL start point sets (S, N, 3) against one target
    (float64), one enqueue and one synchronisation.  Returns (transforms (S,4,4), costs (S,)[, histories (S,n_iter)]).
    target_faces (F,3) switches to on_surface=True (ICP:106-107): target_points are then the target mesh's vertices and
    every source point is matched to the closest point on the triangles."""
    lib = L.lib()
    src = torch.as_tensor(np.ascontiguousarray(np.asarray(start_points, np.float64))).to(device)
    tgt = torch.as_tensor(np.ascontiguousarray(np.asarray(target_points, np.float64))).to(device)
    if src.dim() != 3 or src.shape[2] != 3 or tgt.dim() != 2 or tgt.shape[1] != 3:
        raise L.FohoError("icp_points_multi: expected (S,N,3) start points and (M,3) target points")
    S, N, M = src.shape[0], src.shape[1], tgt.shape[0]
    tf = None
    if target_faces is not None:
        tf = torch.as_tensor(np.ascontiguousarray(np.asarray(target_faces, np.int32))).to(device)
        if tf.dim() != 2 or tf.shape[1] != 3 or tf.shape[0] < 1:
            raise L.FohoError("icp_points_multi: target_faces must be (F,3)")
        if int(tf.min()) < 0 or int(tf.max()) >= M:
            raise L.FohoError("icp_points_multi: target face index out of range")
        nws = lib.foho_icp_surface_workspace_bytes(S, N, tf.shape[0])
    else:
        nws = lib.foho_icp_batch_workspace_bytes(S, N, M)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=device)
    T = torch.zeros(S, 16, dtype=torch.float64, device=device)
    cost = torch.zeros(S, dtype=torch.float64, device=device)
    hist = torch.zeros(S, max(n_iter, 1), dtype=torch.float64, device=device)
    tail = (int(n_iter), int(n_outliers), int(bool(fixed_scale)), min_scale, max_scale, _p(T), _p(cost), _p(hist), _p(ws), nws,
            _stream(src.device))
    if tf is not None:
        L.check(lib.foho_icp_run_surface(_p(src), S, N, _p(tgt), M, _p(tf), int(tf.shape[0]), *tail),
                "foho_icp_run_surface")
    else:
        L.check(lib.foho_icp_run_batch(_p(src), S, N, _p(tgt), M, *tail), "foho_icp_run_batch")
    out = (T.cpu().numpy().reshape(S, 4, 4), cost.cpu().numpy())      # the copies synchronise
    return out + (hist.cpu().numpy()[:, :n_iter],) if return_history else out


def icp_points(source_points, target_points, n_iter, n_outliers=0, fixed_scale=False, min_scale=0.5, max_scale=2.0,
               device="cuda", return_history=False, target_faces=None):
    """One start of icp_points_multi.  Returns (best_transform (4,4) np.float64, best_cost float[, cost history])."""
    out = icp_points_multi(np.asarray(source_points, np.float64)[None], target_points, n_iter, n_outliers, fixed_scale,
                           min_scale, max_scale, device, return_history, target_faces)
    return (out[0][0], float(out[1][0])) + ((out[2][0],) if return_history else ())


# ------------------------------------------------------------------------------------------------ iso-surfacing
class _FlexiFn(torch.autograd.Function):
    """kaolin FlexiCubes.__call__ with default weights (pipelines.py:1393, 1509): differentiable w.r.t. the SDF and the
    grid positions through the edge crossings."""

    @staticmethod
    def forward(ctx, x, s, res, verts_cap, faces_cap):
        _need_cuda(x, s)
        lib = L.lib()
        xx, ss = _f32(x), _f32(s).reshape(-1)
        G = res + 1
        if xx.shape != (G ** 3, 3) or ss.numel() != G ** 3:
            raise L.FohoError(f"flexicubes: expected {(G ** 3, 3)} grid positions and {G ** 3} SDF values")
        dev = xx.device
        nws = lib.foho_flexi_workspace_bytes(res)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        counts = torch.zeros(3, dtype=torch.int32, device=dev)
        while True:
            verts = torch.empty(verts_cap, 3, device=dev)
            faces = torch.empty(faces_cap, 3, dtype=torch.int64, device=dev)
            ldev = torch.empty(verts_cap, device=dev)
            L.check(lib.foho_flexi_fwd(_p(xx), _p(ss), res, _p(verts), verts_cap, _p(faces), faces_cap, _p(ldev), _p(counts), _p(ws), nws,
                                       _stream(dev)), "foho_flexi_fwd")
            nv, nf, over = counts.tolist()           # the output sizes are data dependent: one host sync per extraction
            if not over:
                break
            verts_cap, faces_cap = max(verts_cap, nv), max(faces_cap, nf)
        ctx.save_for_backward(xx, ss)
        ctx.res, ctx.ws, ctx.nv = res, ws, nv
        ctx.need_x = x.requires_grad
        ctx.s_meta, ctx.x_meta = (s.shape, s.dtype), (x.shape, x.dtype)
        f_out, l_out = faces[:nf], ldev[:nv]
        ctx.mark_non_differentiable(f_out, l_out)
        return verts[:nv], f_out, l_out

    @staticmethod
    def backward(ctx, g_verts, _gf, _gl):
        xx, ss = ctx.saved_tensors
        lib = L.lib()
        g = _f32(g_verts)
        gs = torch.zeros_like(ss)
        gx = torch.zeros_like(xx) if ctx.need_x else None
        L.check(lib.foho_flexi_bwd(_p(xx), _p(ss), ctx.res, _p(g), ctx.nv, _p(gs), _p(gx), _p(ctx.ws), ctx.ws.numel(), _stream(xx.device)),
                "foho_flexi_bwd")
        # gradients in the shape and dtype the caller's tensors have (a (G,G,G) or half-precision SDF is a legal input)
        gs = gs.view(ctx.s_meta[0]).to(ctx.s_meta[1])
        if gx is not None:
            gx = gx.view(ctx.x_meta[0]).to(ctx.x_meta[1])
        return gx, gs, None, None, None


def flexicubes(x, s, res, verts_cap=None, faces_cap=None):
    """(verts (V,3), faces (F,3) int64, l_dev (V,)) of the zero level set of s on the regular (res+1)^3 grid x."""
    verts_cap = verts_cap or 16 * res * res
    faces_cap = faces_cap or 32 * res * res
    return _FlexiFn.apply(x, s, int(res), int(verts_cap), int(faces_cap))
