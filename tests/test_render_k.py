"""The fused K-fragment render (ops.render_k_fwd / render_k / render_k_alpha, foho_rastk_render_fwd / _bwd):
mesh -> blended image -> vertex and attribute gradients without the (H,W,K) planes.

Forward: bitwise ops.blend_k_fwd on the planes of ops.raster_k_fwd -- one copy of the arithmetic, the same key order at the cut, so no
tolerance, tie pixels included.  Backward: the measure and the bound of test_blend_k.py::test_through_the_rasteriser_to_the_vertices --
referee ops.raster_k -> the torch route in float64, yardstick the same route in float32, bound BK.bound(yardstick) = 4 x yardstick floored
at 16 float32 ulps, error max |got - ref| / max |ref| per tensor.  The composed route's own error is printed beside the fused one's.

Scenes and K.  The bit-for-bit matrix runs every scene at the K of SCENE_KS, for which the CPU test below shows that some pixel holds
more than K fragments (the cut decides) and some pixel none; K in {1, 3, 8, 9, 32, 33, 100, 128} is covered by long_lists, whose stacked
tile holds far more than 128.  The gradient cases take the issue's K in {4, 8, 100} on two_spheres and near_plane, as the composed
route's own test does; there a pixel at or near the cut and pure padding are asserted on the planes.

Closest to its bound: near_plane, K = 100, sigma = 1e-3, gamma = 1, grad_face_attr -- three faces, every entry the sum of thousands of
pixels' float atomics, against the floor of 1.9e-6.  Seven runs on an MI355X gave 5.4e-7 .. 1.4e-6 (the composed route 2.9e-7 .. 8.9e-7):
the spread is the order of the additions."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_k_ref as BK  # noqa: E402
import rastk_ref as RK  # noqa: E402
from followmyhold_amd import _lib, ops  # noqa: E402
from followmyhold_amd import facade as p3d  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "followmyhold_amd", "csrc")
vp = ctypes.c_void_p
BLUR = 1e-3
FRAMES = [(64, 64), (44, 77)]
K_ALL = [1, 3, 8, 9, 32, 33, 100, 128]           # both slab-class boundaries (8 | 9, 32 | 33) and the largest
# scene -> (frames, K of the bit-for-bit matrix): every K is below the scene's deepest pixel (test_scenes_exercise_the_cut...).
# long_lists' covering triangle leaves no pixel of a square frame empty; the wide frame has empty corners.
SCENE_KS = {"two_spheres": (FRAMES, [1, 3]), "long_lists": ([(44, 77)], K_ALL), "near_plane": (FRAMES, [1]), "coplanar_pair": (FRAMES, [1])}


def _scene(name, H, W):
    if name == "two_spheres":
        return RK.two_spheres(H, W)
    if name == "long_lists":
        return RK.long_lists(H, W)
    return RK.near_plane() if name == "near_plane" else RK.coplanar_pair()


# ---------------------------------------------------------------- CPU
def test_header_library_and_every_refusal_names_its_function():
    subprocess.check_call(["make", "-C", CSRC, "-s"])
    L = _lib.rastk()
    header = open(os.path.join(CSRC, "foho_rastk.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.RASTK_SO_PATH], text=True)
    for fn in ("foho_rastk_render_fwd", "foho_rastk_render_bwd"):
        assert re.search(r"FOHO_RASTK_API int " + fn + r"\(", header) and re.search(r" T " + fn + r"\b", exported) and hasattr(L, fn)
    assert L.foho_rastk_version() == 101 and _lib.RASTK_VERSION == 101 and re.search(r"#define FOHO_RASTK_VERSION 101\b", header)
    one, big = vp(256), ctypes.c_size_t(1 << 40)  # a non-null pointer that is never dereferenced: every call below is refused before any launch
    bg = (ctypes.c_float * 4)(0, 0, 0, 0)
    need = L.foho_rastk_workspace_bytes(10, 10, 64, 64, 4, 100)
    assert need > 0

    def call(fn, K=4, D=3, V=10, F=10, H=64, W=64, blur=0.0, rflags=0, sigma=1e-4, gamma=1e-4, znear=0.01, zfar=100.0, bflags=0, cap=100,
             verts=one, faces=one, attr=one, background=bg, a=one, b=one, c=one, ws=one, wb=big):
        # a, b, c: out, counts, overflow | grad_out, grad_verts_ndc, grad_face_attr
        return getattr(L, fn)(verts, faces, V, F, H, W, K, blur, rflags, attr, D, sigma, gamma, znear, zfar, background, bflags, a, b, c, cap,
                              ws, wb, None)

    for fn in ("foho_rastk_render_fwd", "foho_rastk_render_bwd"):
        def refused(status, *words):
            msg = L.foho_rastk_last_error().decode()
            assert status < 0 and msg.startswith(fn + ":") and all(w in msg for w in words), (fn, status, msg)

        for K in (0, 129, -1):
            refused(call(fn, K=K), "K outside 1 .. 128")
        for D in (0, 5):
            refused(call(fn, D=D), "D outside 1 .. 4")
        for kw in (dict(H=0), dict(W=8193), dict(V=0), dict(F=0), dict(H=8192, W=8192)):
            refused(call(fn, **kw), "out of range")
        for cap in (-1, (1 << 30) + 1):
            refused(call(fn, cap=cap), "list_cap")
        refused(call(fn, blur=-1.0), "blur")
        refused(call(fn, blur=float("nan")), "blur")
        for s in (0.0, -1e-4, float("nan")):
            refused(call(fn, sigma=s), "sigma")
            refused(call(fn, gamma=s), "gamma")
        refused(call(fn, znear=1.0, zfar=1.0), "zfar")
        refused(call(fn, znear=2.0, zfar=1.0), "zfar")
        for flags in (4, 8, 1 << 20, -1):
            refused(call(fn, bflags=flags), "unknown flag")
        for flags in (2, 1 << 20, -1):
            refused(call(fn, rflags=flags), "unknown flag")
        for missing in ("verts", "faces", "attr", "background", "a", "ws"):
            refused(call(fn, **{missing: None}), "null")
        refused(call(fn, wb=need - 1), "too small")
        A = _lib.RASTK_BLEND_ALPHA_ONLY
        refused(call(fn, bflags=A, sigma=0.0), "sigma")           # alpha only: sigma still counts, the attributes do not
        refused(call(fn, bflags=A, attr=None, background=None, verts=None), "null")
    fn = "foho_rastk_render_fwd"
    assert call(fn, c=None) < 0 and L.foho_rastk_last_error().decode().startswith(fn + ": null")       # the overflow word is required


def test_a_missing_symbol_is_a_foho_error_that_says_rebuild(monkeypatch):
    subprocess.check_call(["make", "-C", CSRC, "-s"])
    _lib.rastk()
    monkeypatch.setitem(_lib._sides, "rastk", None)            # forget the loaded library: load_side opens it again
    with pytest.raises(_lib.FohoError, match=r"does not export foho_rastk_no_such_entry: rebuild \(make -C followmyhold_amd/csrc\)"):
        _lib.load_side("rastk", dict(_lib._RASTK_SIGNATURES, foho_rastk_no_such_entry=(ctypes.c_int, [])))


def test_ops_refuse_wrong_arguments_before_any_device_work():
    v, f = torch.zeros(6, 3), torch.arange(6).reshape(2, 3)
    attr = torch.zeros(2, 3, 3)
    good = dict(verts_ndc=v, faces=f, H=32, W=32, K=4, blur_radius=0.0, face_attr=attr, sigma=1e-4, gamma=1e-4, znear=0.01, zfar=100.0,
                background=(1.0, 1.0, 1.0))

    def bad(match, exc=ValueError, **kw):
        for fn in (ops.render_k_fwd, ops.render_k):
            with pytest.raises(exc, match=match):
                fn(**dict(good, **kw))

    for K in (0, 129):
        bad("outside 1 .. 128", K=K)
        with pytest.raises(ValueError, match="outside 1 .. 128"):
            ops.render_k_alpha(v, f, 32, 32, K, 0.0, 1e-4)
    bad("out of range", H=0)
    bad("out of range", W=8193)
    bad(r"\(V,3\)", verts_ndc=torch.zeros(6, 2))
    bad(r"\(F,3\)", faces=torch.arange(6))
    bad("contiguous", faces=torch.arange(12).reshape(2, 6)[:, ::2])
    bad("contiguous", faces=f.float())
    bad("blur", blur_radius=-1.0)
    bad("face_attr", face_attr=attr[:, :2])
    bad("face_attr", face_attr=attr.double())
    bad("face_attr", face_attr=None)
    bad("outside 1 .. 4", face_attr=torch.zeros(2, 3, 5))
    bad("face_attr holds 3 faces", face_attr=torch.zeros(3, 3, 3))
    bad("sigma", sigma=0.0)
    bad("gamma", gamma=-1.0)
    bad("zfar", zfar=0.01)
    bad("background", background=(1.0, 1.0))
    with pytest.raises(ValueError, match="sigma"):
        ops.render_k_alpha(v, f, 32, 32, 4, 0.0, 0.0)
    with pytest.raises(ValueError, match="grad_out"):
        ops.render_k_bwd(*[good[k] for k in good], torch.zeros(32, 32, 3), torch.zeros(8, dtype=torch.uint8), 100)
    # right arguments on the CPU: refused as such, by every entry
    bad("CUDA", exc=_lib.FohoError)
    with pytest.raises(_lib.FohoError, match="CUDA"):
        ops.render_k_alpha(v, f, 32, 32, 4, 0.0, 1e-4)
    with pytest.raises(_lib.FohoError, match="CUDA"):
        ops.render_k_bwd(*[good[k] for k in good], torch.zeros(32, 32, 4), torch.zeros(8, dtype=torch.uint8), 100)
    # the facade's refusals need no device either
    cams = p3d.FoVPerspectiveCameras(device="cpu")
    k_rs, plain_rs = p3d.RasterizationSettings(32, BLUR, 4, k_fragments=True), p3d.RasterizationSettings(32, BLUR, 4)
    fused, unfused = p3d.BlendParams(fused=True), p3d.BlendParams()
    assert p3d.MeshRenderer(p3d.MeshRasterizer(cams, plain_rs), p3d.SoftSilhouetteShader()).fused_render is False
    assert p3d.MeshRenderer(p3d.MeshRasterizer(cams, k_rs), p3d.PhongNormalShader(cameras=cams, blend_params=fused), fused_render=True).fused_render

    class OtherShader(p3d.ShaderBase):
        pass

    for rs, shader, match in ((plain_rs, p3d.PhongNormalShader(cameras=cams, blend_params=fused), "k_fragments=True"),
                              (k_rs, p3d.PhongNormalShader(cameras=cams, blend_params=unfused), "fused=True"),
                              (k_rs, p3d.SoftSilhouetteShader(blend_params=unfused), "fused=True"),
                              (k_rs, OtherShader(blend_params=fused), "PhongNormalShader and SoftSilhouetteShader")):
        with pytest.raises(ValueError, match=match):
            p3d.MeshRenderer(p3d.MeshRasterizer(cams, rs), shader, fused_render=True)
    mesh = p3d.Meshes([v], [f])
    with pytest.raises(ValueError, match="k_fragments=True"):
        p3d.render_mesh(mesh, cams, plain_rs, attr, fused)
    with pytest.raises(ValueError, match="fused=True"):
        p3d.render_mesh(mesh, cams, k_rs, attr, unfused)


@pytest.mark.parametrize("name", list(SCENE_KS))
def test_scenes_exercise_the_cut_an_empty_pixel_and_a_long_list(name):
    """oracle.clib.rasterize on the CPU: for every K of the scene's bit-for-bit matrix some pixel receives more than K fragments and some
    pixel none; long_lists' stacked tile holds more faces than one 64-face chunk of the selection loop."""
    frames, ks = SCENE_KS[name]
    for H, W in frames:
        v, f = _scene(name, H, W)
        for blur in (0.0, BLUR):
            p2f = RK.oracle("render_k " + name, v, f, H, W, blur, 160)[0]
            counts = (p2f >= 0).sum(-1)
            assert counts.max() > max(ks), (name, H, W, blur, int(counts.max()))
            assert (counts == 0).any()
            if name == "long_lists":
                deep = np.unravel_index(np.argmax(counts), counts.shape)
                ty, tx = deep[0] // 8, deep[1] // 8
                ids = p2f[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
                assert len(np.unique(ids[ids >= 0])) > 64 and counts.max() > 128


# ---------------------------------------------------------------- GPU
def _dev(v, f):
    return torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()


@gpu
@pytest.mark.parametrize("name", list(SCENE_KS))
def test_forward_is_bitwise_the_blend_of_the_rasterised_planes(name):
    frames, ks = SCENE_KS[name]
    g = torch.Generator().manual_seed(5)
    n = 0
    for H, W in frames:
        v, f = _dev(*_scene(name, H, W))
        attrs = {D: torch.randn(len(f), 3, D, generator=g).cuda() for D in (1, 3, 4)}
        for K in ks:
            for blur in (0.0, BLUR):
                for cull in (False, True):
                    pl = ops.raster_k_fwd(v, f, H, W, K, blur, cull_backfaces=cull)
                    planes = [pl[k] for k in ("pix_to_face", "zbuf", "bary", "dists")]
                    sigma, gamma = BK.REGIMES[n % 3]
                    modes = [(D, unit, False) for D in (1, 3, 4) for unit in (False, True)] + [(1, False, True)]
                    for D, unit, alpha in modes:
                        bg = tuple(0.1 + 0.2 * c for c in range(D))
                        want = ops.blend_k_fwd(*planes, attrs[D], sigma, gamma, BK.ZNEAR, BK.ZFAR, bg, unit_bary=unit, alpha_only=alpha)
                        got = ops.render_k_fwd(v, f, H, W, K, blur, None if alpha else attrs[D], sigma, gamma, BK.ZNEAR, BK.ZFAR, bg,
                                               cull_backfaces=cull, unit_bary=unit, alpha_only=alpha)
                        what = (name, H, W, K, blur, cull, D, unit, alpha)
                        assert got["out"].shape == want.shape and got["out"].dtype == torch.float32, what
                        assert torch.equal(got["out"], want), (what, float((got["out"] - want).abs().max()))
                        assert got["counts"].dtype == torch.int32 and torch.equal(got["counts"], pl["counts"]), what
                        assert got["workspace"].dtype == torch.uint8 and got["workspace"].is_cuda
                        n += 1
                    if not cull:
                        assert int(pl["counts"].max()) > K and int(pl["counts"].min()) == 0      # the cut decided, and pure padding
    assert n >= 7 * 4 * len(ks)


@functools.lru_cache(maxsize=None)
def _grad_case(name, H, W, K, regime, mode):
    """One gradient case on the device, each route once: dict route -> dict(out, grad_verts[, grad_face_attr]).  Routes: 'ref' (float64
    torch on ops.raster_k's planes), 'f32' (the same in float32), 'composed' (ops.raster_k -> ops.blend_k), 'fused' (ops.render_k) and
    'again' (ops.render_k a second time)."""
    sigma, gamma = BK.REGIMES[regime]
    v, f = _scene(name, H, W)
    df = torch.from_numpy(f).cuda()
    g = torch.Generator().manual_seed(3 + K)
    attr0 = torch.randn(len(f), 3, 3, generator=g).cuda()
    bg = (0.2, 0.5, 0.9)
    alpha, unit = mode == "alpha", mode == "unit"
    gout = torch.randn((H, W) if alpha else (H, W, 4), generator=g).cuda()

    def run(route):
        dv = torch.from_numpy(v).cuda().requires_grad_(True)
        dtype = torch.float64 if route == "ref" else torch.float32
        attr = attr0.to(dtype).clone().requires_grad_(not alpha)          # a leaf of its own: .to() of the same dtype is no copy
        if route in ("fused", "again"):
            if alpha:
                out = ops.render_k_alpha(dv, df, H, W, K, BLUR, sigma)
            else:
                out = ops.render_k(dv, df, H, W, K, BLUR, attr, sigma, gamma, BK.ZNEAR, BK.ZFAR, bg, unit_bary=unit)
        else:
            p2f, z, b, d, _ = ops.raster_k(dv, df, H, W, K, BLUR)
            n_frag = (p2f >= 0).sum(-1)
            assert (n_frag >= min(K, 2)).any() and (n_frag == 0).any()          # layers to blend, and pure padding
            if route == "composed":
                out = ops.blend_k_alpha(p2f, d, sigma) if alpha else ops.blend_k(p2f, z, b, d, attr, sigma, gamma, BK.ZNEAR, BK.ZFAR, bg, unit_bary=unit)
            elif alpha:
                out = BK.torch_alpha(p2f, d, sigma, dtype)
            else:
                out = BK.torch_route(dict(pix_to_face=p2f, zbuf=z, bary=b, dists=d), attr, bg, sigma, gamma, dtype, unit)
        (out * gout.to(out.dtype)).sum().backward()
        res = dict(out=out.detach(), grad_verts=dv.grad)
        if not alpha:
            res["grad_face_attr"] = attr.grad
        return res

    return {r: run(r) for r in ("ref", "f32", "composed", "fused", "again")}


def _check_grads(case, what):
    """Prints yardstick, bound, the fused route's error and the composed route's own beside it, then asserts the fused one."""
    ref, bad = case["ref"], []
    for n in ref:
        assert float(ref[n].abs().max()) > 0 and torch.isfinite(case["fused"][n]).all(), (what, n)
        yard = BK.relerr(case["f32"][n], ref[n])
        lim, err, comp = BK.bound(yard), BK.relerr(case["fused"][n], ref[n]), BK.relerr(case["composed"][n], ref[n])
        print(f"{what} {n}: yardstick {yard:.3g}, bound {lim:.3g}, error {err:.3g}, composed route {comp:.3g}")
        assert case["fused"][n].shape == ref[n].shape and case["fused"][n].dtype == torch.float32
        if not err <= lim:
            bad.append((n, err, lim))
    assert not bad, (what, bad)


GRAD_CASES = [("two_spheres", H, W, K, r, "bary") for H, W in FRAMES for K in (4, 8, 100) for r in (0, 2)] + \
             [("near_plane", 64, 64, K, r, "bary") for K in (4, 8, 100) for r in (0, 2)] + \
             [("two_spheres", 44, 77, 8, 2, "unit"), ("two_spheres", 44, 77, 8, 0, "alpha")]


@gpu
@pytest.mark.parametrize("name,H,W,K,regime,mode", GRAD_CASES)
def test_backward_to_the_vertices_and_the_attributes(name, H, W, K, regime, mode):
    case = _grad_case(name, H, W, K, regime, mode)
    assert torch.equal(case["fused"]["out"], case["composed"]["out"])
    _check_grads(case, f"{name} {H}x{W} K={K} regime={regime} {mode}")


@gpu
def test_overflow_retries_once_at_the_exact_size_with_the_same_bits():
    v, f = _dev(*RK.long_lists(44, 77))
    attr = torch.randn(len(f), 3, 3, generator=torch.Generator().manual_seed(1)).cuda()
    a = [v, f, 44, 77, 33, BLUR, attr, 1e-4, 0.1, BK.ZNEAR, BK.ZFAR, (0.1, 0.2, 0.3)]
    plain, small = ops.render_k_fwd(*a), ops.render_k_fwd(*a, list_cap=16)
    assert small["retried"] and small["list_cap"] > 16 and small["list_cap"] <= plain["list_cap"]
    assert torch.equal(small["out"], plain["out"]) and torch.equal(small["counts"], plain["counts"])
    exact = ops.render_k_fwd(*a, list_cap=small["list_cap"])
    assert not exact["retried"] and torch.equal(exact["out"], plain["out"])


@gpu
def test_repeatable_bitwise_except_the_atomic_gradients():
    case = _grad_case("two_spheres", 64, 64, 8, 2, "bary")
    a, b = case["fused"], case["again"]
    assert torch.equal(a["out"], b["out"])
    v, f = _dev(*RK.two_spheres(64, 64))
    attr = torch.randn(len(f), 3, 3, generator=torch.Generator().manual_seed(1)).cuda()
    r = [ops.render_k_fwd(v, f, 64, 64, 8, BLUR, attr, 1e-3, 1.0, BK.ZNEAR, BK.ZFAR, (0.0, 0.0, 0.0)) for _ in range(2)]
    assert torch.equal(r[0]["out"], r[1]["out"]) and torch.equal(r[0]["counts"], r[1]["counts"])
    for n in ("grad_verts", "grad_face_attr"):
        yard = BK.relerr(case["f32"][n], case["ref"][n])
        err = BK.relerr(a[n], b[n])
        print(f"{n} run to run: yardstick {yard:.3g}, bound {BK.bound(yard):.3g}, difference {err:.3g}")
        assert err <= BK.bound(yard), f"{n} is accumulated with float atomics: two runs may differ by the order of the additions, within " \
                                      f"the bound of the gradient test ({BK.bound(yard):.3g}), not {err:.3g}"


@gpu
def test_backward_computes_only_the_gradients_autograd_asks_for(monkeypatch):
    H = W = 64
    v, f = _dev(*RK.two_spheres(H, W))
    attr = torch.randn(len(f), 3, 3, generator=torch.Generator().manual_seed(1)).cuda()
    L = _lib.rastk()
    real, seen = L.foho_rastk_render_bwd, []

    def spy(*a):
        seen.append([x is not None and (x.value if isinstance(x, vp) else x) is not None for x in a[18:20]])      # grad_verts_ndc, grad_face_attr
        return real(*a)

    monkeypatch.setattr(L, "foho_rastk_render_bwd", spy)

    def grads(need_v, need_a):
        dv, da = v.clone().requires_grad_(need_v), attr.clone().requires_grad_(need_a)
        out = ops.render_k(dv, f, H, W, 8, BLUR, da, 1e-4, 0.1, BK.ZNEAR, BK.ZFAR, (0.1, 0.2, 0.3))
        out.sum().backward()
        return dv.grad, da.grad

    gv, ga = grads(True, False)
    assert seen == [[True, False]] and ga is None and float(gv.abs().max()) > 0
    gv, ga = grads(False, True)
    assert seen[1] == [False, True] and gv is None and float(ga.abs().max()) > 0
    grads(True, True)
    assert seen[2] == [True, True]
    dv = v.clone().requires_grad_(True)
    ops.render_k_alpha(dv, f, H, W, 8, BLUR, 1e-4).sum().backward()
    assert seen[3] == [True, False] and float(dv.grad.abs().max()) > 0


def _peak_over(fn):
    """Increase of torch.cuda.max_memory_allocated over one call of fn, in bytes."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


@gpu
def test_memory_does_not_grow_with_k():
    """64 x 64, K = 128, D = 3: a forward + backward of render_k allocates less than the id plane alone (H W K 8 bytes); the composed
    route, measured the same way, more -- so the measurement sees the planes."""
    H = W = 64
    K = 128
    v, f = _dev(*RK.two_spheres(H, W))
    attr = torch.randn(len(f), 3, 3, generator=torch.Generator().manual_seed(1)).cuda()
    gout = torch.randn(H, W, 4, generator=torch.Generator().manual_seed(2)).cuda()
    a = (1e-4, 0.1, BK.ZNEAR, BK.ZFAR, (0.1, 0.2, 0.3))

    def fused():
        dv, da = v.clone().requires_grad_(True), attr.clone().requires_grad_(True)
        (ops.render_k(dv, f, H, W, K, BLUR, da, *a) * gout).sum().backward()

    def composed():
        dv, da = v.clone().requires_grad_(True), attr.clone().requires_grad_(True)
        p2f, z, b, d, _ = ops.raster_k(dv, f, H, W, K, BLUR)
        (ops.blend_k(p2f, z, b, d, da, *a) * gout).sum().backward()

    fused(), composed()                      # both routes once before the measurement (library load, allocator warm-up)
    id_plane = H * W * K * 8
    got, other = _peak_over(fused), _peak_over(composed)
    print(f"peak bytes over a forward + backward at {H}x{W} K={K}: render_k {got}, raster_k -> blend_k {other}, id plane {id_plane}")
    assert got < id_plane < other


class _SteadyNormals(p3d.Meshes):
    """Meshes whose vertex normals are summed on the host: index_add on the device adds with float atomics, so two renders of one mesh
    would see normals that differ in the last bit, which is not what these tests compare."""

    def verts_normals_packed(self):
        return p3d.Meshes([self._v.cpu()], [self._f.cpu()]).verts_normals_packed().to(self._v.device)


def _facade_scene(H, W):
    from test_raster_k import _scene_mesh
    return _scene_mesh(H, W)


@gpu
@pytest.mark.parametrize("shader", ["phong", "silhouette"])
def test_facade_fused_render_against_the_two_stage_renderer(shader, monkeypatch):
    H, W, K, sigma, gamma = 44, 77, 4, 1e-4, 1e-4
    gout = torch.randn(1, H, W, 4, generator=torch.Generator().manual_seed(9)).cuda()
    calls = []
    real = {n: getattr(ops, n) for n in ("render_k", "render_k_alpha")}
    for n in real:
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **kw: (calls.append(_n), real[_n](*a, **kw))[1])

    def render(route):
        cams, verts, faces = _facade_scene(H, W)
        rast = p3d.MeshRasterizer(cams, p3d.RasterizationSettings((H, W), BLUR, K, k_fragments=True))
        bp = p3d.BlendParams(sigma, gamma, (0.3, 0.6, 0.9), fused=route in ("two_stage", "one"))
        mesh = _SteadyNormals([verts], [faces])
        if route == "ref":                    # the shader's torch route in float64 on the float32 planes
            fr = rast(mesh)
            if shader == "phong":
                img = BK.torch_route(dict(pix_to_face=fr.pix_to_face[0], zbuf=fr.zbuf[0], bary=fr.bary_coords[0], dists=fr.dists[0]),
                                     mesh.verts_normals_packed()[faces], bp.background_color, sigma, gamma, torch.float64, True, cams.znear,
                                     cams.zfar)[None]
            else:
                a = BK.torch_alpha(fr.pix_to_face, fr.dists, sigma, torch.float64)
                img = torch.cat([torch.ones(a.shape + (3,), device="cuda", dtype=torch.float64), a[..., None]], -1)
        else:
            sh = (p3d.PhongNormalShader if shader == "phong" else p3d.SoftSilhouetteShader)(cameras=cams, blend_params=bp)
            img = p3d.MeshRenderer(rast, sh, fused_render=route == "one")(mesh)
        (img * gout.to(img.dtype)).sum().backward()
        return dict(out=img.detach(), grad_verts=verts.grad)

    ref, plain, two = render("ref"), render("torch"), render("two_stage")
    assert not calls                                           # fused_render=False: neither operator is called
    one = render("one")
    assert calls == ["render_k" if shader == "phong" else "render_k_alpha"]
    assert one["out"].shape == (1, H, W, 4) and one["out"].dtype == torch.float32
    assert torch.equal(one["out"], two["out"])
    yard = BK.relerr(plain["grad_verts"], ref["grad_verts"])
    err, comp = BK.relerr(one["grad_verts"], ref["grad_verts"]), BK.relerr(two["grad_verts"], ref["grad_verts"])
    print(f"facade {shader} grad_verts: yardstick {yard:.3g}, bound {BK.bound(yard):.3g}, error {err:.3g}, two-stage renderer {comp:.3g}")
    assert torch.isfinite(one["grad_verts"]).all() and float(ref["grad_verts"].abs().max()) > 0 and err <= BK.bound(yard)


@gpu
def test_facade_default_route_is_unchanged_and_render_mesh_equals_blend_fragments():
    H, W, K = 44, 77, 4
    cams, verts, faces = _facade_scene(H, W)
    mesh = _SteadyNormals([verts], [faces])
    with torch.no_grad():
        # the default renderer (fused_render=False) is the rasteriser, then the shader, with the shader's sigma handed over: on the
        # one-fragment route, on K-fragment planes, blended in torch and by ops.blend_k
        for k_fragments in (False, True):
            rast = p3d.MeshRasterizer(cams, p3d.RasterizationSettings((H, W), BLUR, K, k_fragments=k_fragments))
            for fused in ((False, True) if k_fragments else (False,)):
                bp = p3d.BlendParams(1e-4, 1e-4, (0.3, 0.6, 0.9), fused=fused)
                for sh in (p3d.PhongNormalShader(cameras=cams, blend_params=bp), p3d.SoftSilhouetteShader(blend_params=bp)):
                    got = p3d.MeshRenderer(rast, sh)(mesh)
                    want = sh(rast(mesh, sigma=bp.sigma), mesh, sigma=bp.sigma)
                    assert got.shape == (1, H, W, 4) and torch.equal(got, want), (k_fragments, fused, type(sh).__name__)
        rs = p3d.RasterizationSettings((H, W), BLUR, K, k_fragments=True)
        attr = torch.randn(len(faces), 3, 3, generator=torch.Generator().manual_seed(4)).cuda()
        bp = p3d.BlendParams(1e-4, 0.1, (0.3, 0.6, 0.9), fused=True)
        want = p3d.blend_fragments(p3d.MeshRasterizer(cams, rs)(mesh), attr, bp, cams.znear, cams.zfar)
        got = p3d.render_mesh(mesh, cams, rs, attr, bp)
        assert got.shape == (1, H, W, 4) and torch.equal(got, want) and float((got[..., 3] > 0).sum()) > 100
