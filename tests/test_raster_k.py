"""The K-fragment rasteriser (libfoho_rastk.so, ops.raster_k_fwd / raster_k, RasterizationSettings(k_fragments=True)).

The yardstick is oracle.clib.rasterize(face_verts, H, W, blur, K=K): all four planes equal it bit for bit on every pixel that holds no
two fragments of exactly equal depth (the scenes hold none: the CPU tests count them).  CPU: the library and its exports, argument
validation, and the numpy restatement of the (z, face id, sub) select-and-sort against the oracle on the test scenes.  GPU: oracle
identity over K, frames and blur radii, K = 1 against ops.raster_fwd, long tile lists with the overflow retry, the near plane, a
constructed tie, cull_backfaces, repeatability, the backward pass against K calls of ops.raster_bwd, and the facade."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rastk_ref as RK  # noqa: E402
from followmyhold_amd import _lib, ops  # noqa: E402
from followmyhold_amd import facade as p3d  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "followmyhold_amd", "csrc")
BLUR = RK.BLUR
FRAMES = [(64, 64), (44, 77)]          # 44 x 77: non-square, neither side a multiple of the 8-pixel tile
KS = [1, 2, 4, 8, 100]
vp = ctypes.c_void_p


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = sorted(l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3 and l.split()[-2] in ("T", "t", "W", "V", "B", "D"))
    return [n for n in names if not n.startswith(("_init", "_fini", "__bss_start", "_edata", "_end", "__hip_"))]


# ---------------------------------------------------------------- CPU
def test_rastk_library_builds_and_exports_exactly_its_header():
    subprocess.check_call(["make", "-C", CSRC, "-s"])
    assert os.path.exists(_lib.RASTK_SO_PATH)
    from test_cabi import declared_functions as _declared
    want = _declared(os.path.join(CSRC, "foho_rastk.h"))
    assert {"foho_rastk_version", "foho_rastk_workspace_bytes", "foho_rastk_fwd", "foho_rastk_bwd", "foho_rastk_last_error"} <= set(want)
    assert _exported(_lib.RASTK_SO_PATH) == want
    # the three other libraries export what their headers declare, as before: nothing of this one leaked into them
    here = os.path.dirname(_lib.RASTK_SO_PATH)
    assert _exported(os.path.join(here, "libfoho_vol.so")) == _declared(os.path.join(CSRC, "foho_vol.h"))
    assert _exported(os.path.join(here, "libfoho_sflexi.so")) == _declared(os.path.join(CSRC, "foho_sflexi.h"))
    hip = _exported(_lib.SO_PATH)
    assert hip == _declared() and not [n for n in hip if "rastk" in n]


def test_binding_and_ops_validate_arguments_without_a_gpu():
    subprocess.check_call(["make", "-C", CSRC, "-s"])
    L = _lib.rastk()
    assert L.foho_rastk_version() == _lib.RASTK_VERSION
    one, big = vp(256), ctypes.c_size_t(1 << 40)      # a non-null pointer that is never dereferenced: every call is refused before any launch

    def fwd(K=4, H=64, W=64, V=10, F=10, cap=100, flags=0, blur=0.0, verts=one, ov=one, ws=one, wb=big):
        return L.foho_rastk_fwd(verts, one, V, F, H, W, K, blur, flags, one, one, one, one, one, ov, cap, ws, wb, None)

    def refused(status, *words):
        msg = L.foho_rastk_last_error().decode()
        assert status < 0 and all(w in msg for w in words), (status, msg)

    for K in (0, 129, -1):
        refused(fwd(K=K), "foho_rastk_fwd", "K outside")
        refused(L.foho_rastk_bwd(one, one, 10, 10, 64, 64, K, one, None, None, None, one, 0.0, None), "foho_rastk_bwd", "K outside")
        assert L.foho_rastk_workspace_bytes(10, 10, 64, 64, K, 100) == 0
    refused(fwd(verts=None), "null")
    refused(fwd(ov=None), "null")
    refused(fwd(H=0), "out of range")
    refused(fwd(W=8193), "out of range")
    refused(fwd(cap=-1), "list_cap")
    refused(fwd(flags=2), "flag")
    refused(fwd(blur=-1.0), "blur")
    need = L.foho_rastk_workspace_bytes(10, 10, 64, 64, 4, 100)
    assert need > 0 and L.foho_rastk_workspace_bytes(10, 10, 64, 64, 4, 100100) >= need + 4 * 100000 - 256      # 4 B per list entry, 256-B regions
    refused(fwd(wb=need - 1), "too small")
    # the Python operators refuse before any device work (CPU tensors here: a device call would raise FohoError("... need CUDA"))
    assert p3d.RasterizationSettings(k_fragments=True).k_fragments and not p3d.RasterizationSettings().k_fragments
    v, f = torch.zeros(6, 3), torch.arange(6).reshape(2, 3)
    for K in (0, 129):
        with pytest.raises(ValueError, match="outside 1 .. 128"):
            ops.raster_k_fwd(v, f, 32, 32, K, 0.0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.raster_k_fwd(v, torch.arange(12).reshape(2, 6)[:, ::2], 32, 32, 4, 0.0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.raster_k_fwd(v, f.float(), 32, 32, 4, 0.0)
    with pytest.raises(_lib.FohoError, match="CUDA"):
        ops.raster_k_fwd(v, f, 32, 32, 4, 0.0)


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("blur", [0.0, BLUR])
def test_scenes_are_tie_free_and_the_key_rule_restates_the_oracle(H, W, blur):
    """No pixel of the jittered scene holds two fragments of equal depth (change the seed if one ever does, never the cap), and on
    such a scene sorting the oracle's whole fragment set by (z, face id) and cutting at K is the oracle's K-buffer, for every K of
    the GPU tests.  The scene exercises the cut (K below the deepest pixel), K equal to a pixel's count, and pure padding."""
    v, f = RK.two_spheres(H, W)
    full = RK.oracle("two_spheres", v, f, H, W, blur, RK.K_ALL)
    counts = (full[0] >= 0).sum(-1)
    assert counts.max() < RK.K_ALL and int(RK.tie_pixels(full[0], full[1]).sum()) == 0
    assert counts.max() > 2 and counts.max() < 100 and (counts == 2).any() and (counts == 4).any() and (counts == 0).any()
    for K in KS:
        ref = RK.oracle("two_spheres", v, f, H, W, blur, K)
        for a, b in zip(RK.select_sort(full, K), ref):
            assert np.array_equal(a, b), K


def test_key_rule_on_the_culled_and_near_plane_scenes():
    H, W = FRAMES[0]
    v, f = RK.two_spheres(H, W)
    full = RK.oracle("two_spheres", v, f, H, W, BLUR, RK.K_ALL, cull=True)
    assert int(RK.tie_pixels(full[0], full[1]).sum()) == 0
    assert (full[0] >= 0).sum() < (RK.oracle("two_spheres", v, f, H, W, BLUR, RK.K_ALL)[0] >= 0).sum()     # back faces are gone
    for a, b in zip(RK.select_sort(full, 2), RK.oracle("two_spheres", v, f, H, W, BLUR, 2, cull=True)):
        assert np.array_equal(a, b)
    v, f = RK.near_plane()
    full = RK.oracle("near_plane", v, f, 96, 96, BLUR, 4)
    assert int(RK.tie_pixels(full[0], full[1]).sum()) == 0 and (full[0] >= 0).sum(-1).max() in (2, 3)      # K = 4 is above every count
    v, f = RK.long_lists()
    full = RK.oracle("long_lists", v, f, 32, 32, BLUR, 128)
    assert int(RK.tie_pixels(full[0], full[1]).sum()) == 0 and (full[0][..., -1] >= 0).any()               # pixels with >= 128 fragments


# ---------------------------------------------------------------- GPU
def _dev(v, f):
    return torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()


def _assert_equals_oracle(out, ref, what):
    ties = RK.tie_pixels(ref[0], ref[1])
    deep = ((ref[0] >= 0).sum(-1) >= 2).sum()
    assert ties.sum() <= 1e-3 * deep, (what, int(ties.sum()), int(deep))
    ok = ~ties
    for name, r in zip(("pix_to_face", "zbuf", "bary", "dists"), ref):
        got = out[name].cpu().numpy()
        assert got.shape == r.shape and got.dtype == r.dtype, (what, name, got.shape, got.dtype)
        assert np.array_equal(got[ok], r[ok]), (what, name, int((got != r).sum()))


@gpu
@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("blur", [0.0, BLUR])
def test_equals_the_oracle_for_every_k(H, W, blur):
    v, f = RK.two_spheres(H, W)
    dv, df = _dev(v, f)
    full = RK.oracle("two_spheres", v, f, H, W, blur, RK.K_ALL)
    counts = (full[0] >= 0).sum(-1)
    for K in KS:
        out = ops.raster_k_fwd(dv, df, H, W, K, blur)
        _assert_equals_oracle(out, RK.oracle("two_spheres", v, f, H, W, blur, K), (H, W, blur, K))
        assert out["counts"].dtype == torch.int32 and np.array_equal(out["counts"].cpu().numpy(), counts)     # every count is < 128 here


@gpu
def test_k1_equals_raster_fwd_on_hit_pixels():
    H, W = FRAMES[1]
    v, f = RK.two_spheres(H, W)
    dv, df = _dev(v, f)
    a = ops.raster_k_fwd(dv, df, H, W, 1, BLUR)
    b = ops.raster_fwd(dv, df, H, W, BLUR, want_sil=False)
    hit = b["pix_to_face"] >= 0
    assert hit.sum() > 200 and torch.equal(a["pix_to_face"][..., 0], b["pix_to_face"])     # background is -1 in both
    for k in ("zbuf", "dists"):
        assert torch.equal(a[k][..., 0][hit], b[k][hit]), k
        assert (a[k][..., 0][~hit] == -1).all()
    assert torch.equal(a["bary"][:, :, 0][hit], b["bary"][hit]) and (a["bary"][:, :, 0][~hit] == -1).all()


@gpu
def test_long_tile_lists_and_the_overflow_retry():
    v, f = RK.long_lists()
    dv, df = _dev(v, f)
    out = ops.raster_k_fwd(dv, df, 32, 32, 128, BLUR, list_cap=1 << 16)
    assert not out["retried"] and int(out["counts"].max()) > 4 * 128      # the cut is deep: most fragments of the tile's centre are dropped
    _assert_equals_oracle(out, RK.oracle("long_lists", v, f, 32, 32, BLUR, 128), "long lists")
    again = ops.raster_k_fwd(dv, df, 32, 32, 128, BLUR, list_cap=64)          # too small: overflow bit, one retry with the exact size
    assert again["retried"] and 601 <= again["list_cap"] < (1 << 16)
    for k in ("pix_to_face", "zbuf", "bary", "dists", "counts"):
        assert torch.equal(out[k], again[k]), k


def _near_plane_case(flip):
    v, f = RK.near_plane()
    return v, (np.ascontiguousarray(f[:, ::-1]) if flip else f), ("near_plane_flipped" if flip else "near_plane")


def test_cull_on_the_near_plane_scene_removes_each_straddling_face_under_one_winding():
    """cull_backfaces tests the area sign of the sub-triangles: between the scene and its copy with every face's winding reversed,
    each straddling face is on screen under exactly one of the two (the GPU test compares both with the oracle)."""
    seen = []
    for flip in (False, True):
        v, f, name = _near_plane_case(flip)
        p2f = RK.oracle(name, v, f, 96, 96, BLUR, 4, cull=True)[0]
        assert int(RK.tie_pixels(*RK.oracle(name, v, f, 96, 96, BLUR, 4, cull=True)[:2]).sum()) == 0
        seen.append([bool((p2f == i).any()) for i in range(3)])
    assert all(a != b for a, b in zip(*seen)), seen


@gpu
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("cull", [False, True])
def test_near_plane_faces_equal_the_oracle(flip, cull):
    v, f, name = _near_plane_case(flip)
    dv, df = _dev(v, f)
    out = ops.raster_k_fwd(dv, df, 96, 96, 4, BLUR, cull_backfaces=cull)
    ref = RK.oracle(name, v, f, 96, 96, BLUR, 4, cull=cull)
    if not cull:
        assert ((ref[0] == 0).any(-1)).sum() > 100 and ((ref[0] == 1).any(-1)).sum() > 100       # both straddling faces are on screen
    assert (ref[0] >= 0).sum(-1).max() < 4                                                       # K is above every count
    _assert_equals_oracle(out, ref, ("near plane", flip, cull))
    assert np.array_equal(out["counts"].cpu().numpy(), (ref[0] >= 0).sum(-1))


@gpu
def test_constructed_tie_keeps_the_lower_face_id():
    v, f = RK.coplanar_pair()
    dv, df = _dev(v, f)
    one = ops.raster_k_fwd(dv, df, 32, 32, 1, BLUR)["pix_to_face"]
    assert (one >= 0).sum() > 50 and (one[one >= 0] == 0).all()
    assert np.array_equal(one.cpu().numpy(), RK.oracle("coplanar", v, f, 32, 32, BLUR, 1)[0])
    two = ops.raster_k_fwd(dv, df, 32, 32, 2, BLUR)
    hit = two["pix_to_face"][..., 0] >= 0
    assert torch.equal(hit, one[..., 0] >= 0)
    assert (two["pix_to_face"][hit][:, 0] == 0).all() and (two["pix_to_face"][hit][:, 1] == 1).all()
    assert torch.equal(two["zbuf"][hit][:, 0], two["zbuf"][hit][:, 1]) and (two["counts"][hit] == 2).all()


@gpu
@pytest.mark.parametrize("cull", [False, True])
def test_cull_backfaces_equals_the_oracle(cull):
    H, W = FRAMES[0]
    v, f = RK.two_spheres(H, W)
    dv, df = _dev(v, f)
    out = ops.raster_k_fwd(dv, df, H, W, 8, BLUR, cull_backfaces=cull)
    _assert_equals_oracle(out, RK.oracle("two_spheres", v, f, H, W, BLUR, 8, cull=cull), ("cull", cull))


@gpu
def test_forward_is_bitwise_repeatable():
    H, W = FRAMES[1]
    dv, df = _dev(*RK.two_spheres(H, W))
    a, b = (ops.raster_k_fwd(dv, df, H, W, 8, BLUR) for _ in range(2))
    for k in ("pix_to_face", "zbuf", "bary", "dists", "counts"):
        assert torch.equal(a[k], b[k]), k


def _bwd_reference(dv, df, p2f, gz, gb, gd, order, dtype):
    acc = torch.zeros(dv.shape, dtype=dtype, device=dv.device)
    for k in order:
        acc += ops.raster_bwd(dv, df, p2f[..., k].contiguous(), gz[..., k] if gz is not None else None,
                              gb[:, :, k] if gb is not None else None, gd[..., k] if gd is not None else None, blur_radius=BLUR).to(dtype)
    return acc


@gpu
@pytest.mark.parametrize("K", [1, 4])
def test_backward_equals_k_calls_of_raster_bwd(K):
    """Reference: ops.raster_bwd per plane, summed in float64.  Both routes add with float atomics, so the bound is measured: the
    reference against itself (planes in reverse order, summed in float32) gives the spread; the new backward gets 4x that (K
    planes land in one launch), floored at one float32 ulp of the largest gradient magnitude.
    The test prints the spread, the ulp, the tolerance and the error."""
    H, W = FRAMES[0]
    dv, df = _dev(*RK.two_spheres(H, W))
    p2f = ops.raster_k_fwd(dv, df, H, W, K, BLUR)["pix_to_face"]
    g = torch.Generator().manual_seed(5)
    gz = torch.randn(H, W, K, generator=g).cuda()
    gb = torch.randn(H, W, K, 3, generator=g).cuda()
    gd = (torch.randn(H, W, K, generator=g) * 1e3).cuda()
    ref = _bwd_reference(dv, df, p2f, gz, gb, gd, range(K), torch.float64)
    ref2 = _bwd_reference(dv, df, p2f, gz, gb, gd, reversed(range(K)), torch.float32)
    spread = float((ref - ref2.double()).abs().max())
    ulp = float(np.spacing(np.float32(ref.abs().max().item())))
    tol = max(4.0 * spread, ulp)
    got = ops.raster_k_bwd(dv, df, p2f, gz, gb, gd, blur_radius=BLUR)
    err = float((got.double() - ref).abs().max())
    print(f"raster_k_bwd K={K}: max |grad| {float(ref.abs().max()):.6g}, reference spread {spread:.6g}, ulp {ulp:.6g}, "
          f"tolerance {tol:.6g}, error {err:.6g}")
    assert got.shape == dv.shape and got.dtype == torch.float32 and float(ref.abs().max()) > 0
    assert err <= tol, (err, tol, spread, ulp)
    # null gradient pointers: only the distance plane
    only_d = ops.raster_k_bwd(dv, df, p2f, None, None, gd, blur_radius=BLUR)
    ref_d = _bwd_reference(dv, df, p2f, None, None, gd, range(K), torch.float64)
    ref_d2 = _bwd_reference(dv, df, p2f, None, None, gd, reversed(range(K)), torch.float32)
    tol_d = max(4.0 * float((ref_d - ref_d2.double()).abs().max()), float(np.spacing(np.float32(ref_d.abs().max().item()))))
    assert float((only_d.double() - ref_d).abs().max()) <= tol_d
    assert not ops.raster_k_bwd(dv, df, p2f, None, None, None, blur_radius=BLUR).any()
    # a pixel that is -1 in every plane contributes nothing
    empty = (p2f < 0).all(-1)
    assert empty.sum() > 100
    m = empty[..., None].float()
    assert not ops.raster_k_bwd(dv, df, p2f, gz * m, gb * m[..., None], gd * m, blur_radius=BLUR).any()


def _scene_mesh(H, W):
    """The two spheres in world space in front of the facade's camera (its NDC transform runs on the device)."""
    from followmyhold_amd import synthetic
    v, f = synthetic.icosphere(2, 0.4)
    rng = np.random.default_rng(11)
    vv = np.concatenate([v, v * np.float32(0.7) + np.array([0.12, 0.06, 0.05], np.float32)]).astype(np.float32)
    vv = vv + rng.normal(scale=0.004, size=vv.shape).astype(np.float32) + np.array([0.05, -0.02, -2.0], np.float32)
    Rm = torch.tensor([[-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]], device="cuda").unsqueeze(0)
    cams = p3d.FoVPerspectiveCameras(device="cuda", R=Rm, T=torch.zeros(1, 3, device="cuda"), znear=0.01, zfar=100.0, fov=50.0)
    verts = torch.from_numpy(vv).cuda().requires_grad_(True)
    return cams, verts, torch.from_numpy(np.concatenate([f, f + len(v)]).astype(np.int64)).cuda()


@gpu
def test_facade_k_fragments():
    H = W = 64
    K = 4
    cams, verts, faces = _scene_mesh(H, W)
    mesh = p3d.Meshes([verts], [faces])
    blend = p3d.BlendParams(sigma=1e-4, gamma=1e-4)
    rast = p3d.MeshRasterizer(cams, p3d.RasterizationSettings((H, W), BLUR, K, k_fragments=True))
    frag = rast(mesh)
    assert frag.sil_prod is None and frag.pix_to_face.shape == (1, H, W, K) and frag.pix_to_face.dtype == torch.int64
    assert frag.zbuf.shape == (1, H, W, K) and frag.dists.shape == (1, H, W, K) and frag.bary_coords.shape == (1, H, W, K, 3)
    # the oracle on the NDC vertices the facade's camera produced, moved to the device
    ndc = rast.transform(mesh).detach().cpu().numpy()
    ref = RK.oracle("facade", ndc, faces.cpu().numpy(), H, W, BLUR, K)
    assert int(RK.tie_pixels(ref[0], ref[1]).sum()) == 0 and ((ref[0] >= 0).sum(-1) == K).any()
    o = [torch.from_numpy(a).cuda()[None] for a in ref]
    ofrag = p3d.Fragments(o[0], o[1], o[2], o[3], None)
    for a, b in ((frag.pix_to_face, ofrag.pix_to_face), (frag.zbuf, ofrag.zbuf), (frag.bary_coords, ofrag.bary_coords), (frag.dists, ofrag.dists)):
        assert torch.equal(a.detach(), b)
    phong = p3d.PhongNormalShader(cameras=cams, blend_params=blend)
    with torch.no_grad():
        # softmax_rgb_blend over the K layers.  The face attributes are formed ONCE and shared: Meshes.verts_normals_packed sums with
        # index_add (float atomics on the device), so two shader calls see vertex normals that differ in the last bit.
        face_normals = mesh.verts_normals_packed()[faces]

        def shade(fr):
            colors = p3d.interpolate_face_attributes(fr.pix_to_face, fr.bary_coords, face_normals)
            return p3d.softmax_rgb_blend(colors, fr, blend, znear=cams.znear, zfar=cams.zfar)

        img_hip, img_ref = shade(frag), shade(ofrag)
        assert img_hip.shape == (1, H, W, 4) and torch.isfinite(img_hip).all() and torch.equal(img_hip, img_ref)
        assert float((img_hip[..., :3] - 1.0).abs().max()) > 0.1          # not all background
        sil =p3d.SoftSilhouetteShader(blend_params=blend)
        alpha = sil(frag, mesh)[..., 3]
        want = 1.0 - torch.prod(1.0 - torch.sigmoid(-ofrag.dists / blend.sigma) * (ofrag.pix_to_face >= 0), dim=-1)
        assert torch.equal(alpha, want) and 0 < float(alpha.sum()) < H * W
    # differentiable through the rasteriser: zbuf, barycentrics and distances all carry gradient to the vertices
    img = p3d.MeshRenderer(rast, phong)(mesh)
    fr = rast(mesh)
    hit = fr.pix_to_face >= 0
    loss = img[..., :3].square().mean() + fr.zbuf[hit].mean() + (fr.bary_coords[hit] * torch.tensor([1.0, 2.0, 3.0], device="cuda")).mean()
    loss.backward()
    assert torch.isfinite(verts.grad).all() and float(verts.grad.abs().max()) > 0
    # k_fragments=False: the shapes and the silhouette plane of before
    for K0, sp in ((1, None), (K, (1, H, W))):
        fr0 = p3d.MeshRasterizer(cams, p3d.RasterizationSettings((H, W), BLUR, K0))(mesh)
        assert fr0.pix_to_face.shape == (1, H, W, 1) and fr0.zbuf.shape == (1, H, W, 1) and fr0.bary_coords.shape == (1, H, W, 1, 3)
        assert (fr0.sil_prod is None) if sp is None else (tuple(fr0.sil_prod.shape) == sp)
    with pytest.raises(ValueError, match="faces_per_pixel > 1"):
        p3d.SoftSilhouetteShader(blend_params=blend)(p3d.MeshRasterizer(cams, p3d.RasterizationSettings((H, W), BLUR, 1))(mesh), mesh)
    with pytest.raises(ValueError, match="faces_per_pixel > 1"):
        p3d.SoftSilhouetteShader(blend_params=blend)(p3d.MeshRasterizer(cams, p3d.RasterizationSettings((H, W), BLUR, 1, k_fragments=True))(mesh), mesh)
