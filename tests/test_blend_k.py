"""Fused shading and blending of K-fragment planes (foho_rastk_blend_fwd / _bwd, ops.blend_k / blend_k_alpha, BlendParams(fused=True)).

Referee, yardstick, measure and bound: tests/blend_k_ref.py -- the facade's torch route in float64, the same route in float32 against it,
max |got - ref| / max |ref| per tensor, 4 x yardstick floored at 16 float32 ulps (1.9e-6).  Every comparison prints its yardstick,
bound and error.  CPU: version, refusals, argument checks, the constructed planes' properties, the referee against the float32 route.
GPU: constructed planes over K, D and the three (sigma, gamma) regimes; saturated layers; the front-packed contract; through the
rasteriser to the vertices; flags and facade; repeatability; needs-grad pruning.

Measured on an MI355X (largest error / its bound over all tensors of a test): see DESIGN.md section 3C."""
import ctypes
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
from followmyhold_amd.ops import blend_k, blend_k_alpha, blend_k_bwd, blend_k_fwd  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "followmyhold_amd", "csrc")
KS = [1, 3, 8, 100, 128]
DS = [1, 3, 4]
vp = ctypes.c_void_p
FLOATS = ("zbuf", "bary", "dists", "face_attr")


# ---------------------------------------------------------------- CPU
def test_version_101_and_every_refusal_names_its_function():
    subprocess.check_call(["make", "-C", CSRC, "-s"])
    L = _lib.rastk()
    header = open(os.path.join(CSRC, "foho_rastk.h")).read()
    assert L.foho_rastk_version() == 101 and _lib.RASTK_VERSION == 101 and _lib.SIDE_VERSIONS["rastk"] == 101
    assert re.search(r"#define FOHO_RASTK_VERSION 101\b", header) and "FRONT-PACKED" in header
    one = vp(256)                  # a non-null pointer that is never dereferenced: every call below is refused before any launch
    bg = (ctypes.c_float * 4)(0, 0, 0, 0)

    def call(fn, K=4, D=3, F=10, H=8, W=8, sigma=1e-4, gamma=1e-4, znear=0.01, zfar=100.0, flags=0, p2f=one, zbuf=one, bary=one, dists=one,
             attr=one, background=bg, last=one):
        head = (p2f, zbuf, bary, dists, attr, F, H, W, K, D, sigma, gamma, znear, zfar, background, flags)
        if fn == "foho_rastk_blend_fwd":
            return L.foho_rastk_blend_fwd(*head, last, None)
        return L.foho_rastk_blend_bwd(*head, last, one, one, one, one, None)

    for fn in ("foho_rastk_blend_fwd", "foho_rastk_blend_bwd"):
        def refused(status, *words):
            msg = L.foho_rastk_last_error().decode()
            assert status < 0 and msg.startswith(fn + ":") and all(w in msg for w in words), (fn, status, msg)

        for K in (0, 129, -1):
            refused(call(fn, K=K), "K outside 1 .. 128")
        for D in (0, 5):
            refused(call(fn, D=D), "D outside 1 .. 4")
        for s in (0.0, -1e-4, float("nan")):
            refused(call(fn, sigma=s), "sigma")
            refused(call(fn, gamma=s), "gamma")
        refused(call(fn, znear=1.0, zfar=1.0), "zfar")
        refused(call(fn, znear=2.0, zfar=1.0), "zfar")
        for flags in (4, 8, 1 << 20, -1):
            refused(call(fn, flags=flags), "unknown flag")
        refused(call(fn, H=0), "out of range")
        refused(call(fn, F=0), "out of range")
        for missing in ("p2f", "zbuf", "bary", "dists", "attr", "background", "last"):
            refused(call(fn, **{missing: None}), "null")
        # what the flags make optional is optional, what they do not is still required
        U, A = _lib.RASTK_BLEND_UNIT_BARY, _lib.RASTK_BLEND_ALPHA_ONLY
        refused(call(fn, flags=U, zbuf=None), "null")
        refused(call(fn, flags=A, dists=None), "null")
        refused(call(fn, flags=A, sigma=0.0), "sigma")
        refused(call(fn, flags=A, last=None), "null")


def test_ops_refuse_wrong_arguments_before_any_device_work():
    assert p3d.BlendParams().fused is False and p3d.BlendParams(fused=True).fused is True
    c = BK.constructed(3, 3, 1e-4)
    a = [c["pix_to_face"], c["zbuf"], c["bary"], c["dists"], c["face_attr"], 1e-4, 1e-4, BK.ZNEAR, BK.ZFAR, c["background"]]

    def bad(i, v, match, exc=ValueError):
        b = list(a)
        b[i] = v
        for fn in (blend_k_fwd, blend_k, lambda *x: blend_k_bwd(*x, c["grad_out"])):
            with pytest.raises(exc, match=match):
                fn(*b)

    bad(0, c["pix_to_face"].int(), "int64")
    bad(0, c["pix_to_face"][0], "int64")
    bad(1, c["zbuf"][:, :, :2], "zbuf")
    bad(1, c["zbuf"].double(), "zbuf")
    bad(2, c["bary"][..., :2], "bary")
    bad(3, c["dists"].half(), "dists")
    bad(4, c["face_attr"][:, :2], "face_attr")
    bad(4, torch.zeros(5, 3, 5), "outside 1 .. 4")
    bad(5, 0.0, "sigma")
    bad(6, -1.0, "gamma")
    bad(8, BK.ZNEAR, "zfar")
    bad(9, (1.0, 1.0), "background")
    with pytest.raises(ValueError, match="outside 1 .. 128"):
        blend_k_alpha(torch.zeros(2, 2, 129, dtype=torch.int64), torch.zeros(2, 2, 129), 1e-4)
    with pytest.raises(ValueError, match="grad_out"):
        blend_k_bwd(*a, c["grad_out"][..., :2])
    # right arguments on the CPU: refused as such, by every entry
    for fn in (blend_k_fwd, blend_k, lambda *x: blend_k_bwd(*x, c["grad_out"])):
        with pytest.raises(_lib.FohoError, match="CUDA"):
            fn(*a)
    with pytest.raises(_lib.FohoError, match="CUDA"):
        blend_k_alpha(c["pix_to_face"], c["dists"], 1e-4)
    # the facade: fused=True refuses planes that are not K-fragment planes, in every shader and in blend_fragments
    one = p3d.Fragments(c["pix_to_face"][None], c["zbuf"][None], c["bary"][None], c["dists"][None], None)
    assert one.k_planes is False and p3d.Fragments(None, None, None, None, None, k_planes=True).k_planes is True
    fused = p3d.BlendParams(fused=True)
    with pytest.raises(ValueError, match="k_fragments=True"):
        p3d.blend_fragments(one, c["face_attr"], fused, BK.ZNEAR, BK.ZFAR)
    with pytest.raises(ValueError, match="k_fragments=True"):
        p3d.SoftSilhouetteShader(blend_params=fused)(one, None)
    # ... and fused=False is the torch route, which runs where the planes are
    img = p3d.blend_fragments(one, c["face_attr"], p3d.BlendParams(background_color=c["background"]), BK.ZNEAR, BK.ZFAR)
    assert img.shape == (1,) + BK.FRAME + (4,) and torch.isfinite(img).all()


def _delta_clamped(case, gamma):
    """(hit pixels, hit pixels on which softmax_rgb_blend clamps delta), in float64"""
    hit = case["pix_to_face"][..., 0] >= 0
    zinv = (BK.ZFAR - case["zbuf"].double()) / (BK.ZFAR - BK.ZNEAR) * (case["pix_to_face"] >= 0)
    raw = torch.exp((1e-10 - zinv.max(-1).values.clamp(min=1e-10)) / gamma)
    return int(hit.sum()), int((hit & (raw < 1e-10)).sum())


@pytest.mark.parametrize("K", KS)
def test_constructed_planes_have_the_properties_the_gpu_tests_rely_on(K):
    for sigma, gamma in BK.REGIMES:
        c = BK.constructed(K, 3, sigma)
        p2f, z, counts = c["pix_to_face"].numpy(), c["zbuf"].numpy(), c["counts"]
        valid = p2f >= 0
        assert p2f.shape == BK.FRAME + (K,) and (BK.FRAME[0] * BK.FRAME[1]) % 64 and BK.FRAME[1] % 8
        assert {0, min(1, K), K - 1, K} <= set(counts.ravel().tolist())
        # front-packed, -1 padded, ids in range
        assert np.array_equal(valid, np.arange(K) < counts[..., None]) and (p2f[valid] < BK.N_FACES).all()
        assert (z[~valid] == -1).all() and (c["dists"].numpy()[~valid] == -1).all() and (c["bary"].numpy()[~valid] == -1).all()
        # depths strictly increasing in float32 (so tie-free) and inside the clip range
        both = valid[..., 1:]
        assert (np.diff(z, axis=-1)[both] > 0).all() and (z[valid] > BK.ZNEAR).all() and (z[valid] < BK.ZFAR).all()
        hit, clamped = _delta_clamped(c, gamma)
        assert hit > 100 and clamped == (hit if gamma == 1e-4 else 0), (sigma, gamma, hit, clamped)
        x = c["dists"].numpy()[valid] / sigma
        assert (x > 0).sum() > 20 and (x < 0).sum() > 20 and np.abs(x).max() < 15          # both signs; sigmoid far from saturation


def test_saturated_planes_hold_exact_zeros_in_float32():
    c = BK.saturated()
    q = 1.0 - torch.sigmoid(-c["dists"] / 1e-4)                  # float32, as the torch route forms it
    zeros = (q == 0).sum(-1)
    assert int((zeros >= 2).sum()) >= 20 and int((zeros == 1).sum()) >= 20 and int((zeros == 0).sum()) >= 20
    assert int((zeros >= 3).sum()) >= 5 and int(((c["dists"] / 1e-4).abs() >= 0.99e6).sum()) >= 20
    assert ((c["dists"] / 1e-4) >= 0.99e6).any() and ((c["dists"] / 1e-4) <= -0.99e6).any()
    assert (c["pix_to_face"] >= 0).all()


@pytest.mark.parametrize("regime", range(3))
def test_referee_against_the_float32_route_is_finite_and_prints_its_yardsticks(regime):
    sigma, gamma = BK.REGIMES[regime]
    for K in KS:
        for unit in (False, True):
            ref, yard = BK.referee_and_yardstick(("constructed", K, 3), BK.constructed(K, 3, sigma), sigma, gamma, "cpu", unit)
            print(f"CPU yardstick sigma={sigma} gamma={gamma} K={K} unit_bary={unit}: " + ", ".join(f"{n} {y:.3g}" for n, y in yard.items()))
            assert all(torch.isfinite(t).all() for t in ref.values() if t is not None) and all(np.isfinite(y) for y in yard.values())
            assert "out" in yard and "grad_dists" in yard and ("grad_zbuf" in yard or (K == 1 and gamma == 1e-4))
            if K == 1 and gamma == 1e-4:
                assert not ref["grad_zbuf"].any()                 # delta clamped, one fragment: exactly 0
    c = BK.saturated()
    ref, yard = BK.referee_and_yardstick("saturated", c, 1e-4, 1e-4, "cpu")
    print("CPU yardstick saturated: " + ", ".join(f"{n} {y:.3g}" for n, y in yard.items()))
    assert all(torch.isfinite(t).all() for t in ref.values() if t is not None)


# ---------------------------------------------------------------- GPU
def _fused(case, sigma, gamma, unit_bary=False, need=FLOATS):
    """ops.blend_k on the case's planes and its gradients under case['grad_out']: dict over BK.NAMES (None where not asked for)."""
    t = {k: case[k].cuda().requires_grad_(k in need) for k in FLOATS}
    out = blend_k(case["pix_to_face"].cuda(), t["zbuf"], None if unit_bary else t["bary"], t["dists"], t["face_attr"], sigma, gamma,
                  BK.ZNEAR, BK.ZFAR, case["background"], unit_bary=unit_bary)
    keys = [k for k in need if not (unit_bary and k == "bary")]
    g = torch.autograd.grad(out, [t[k] for k in keys], case["grad_out"].cuda())
    res = {n: None for n in BK.NAMES}
    res["out"] = out.detach()
    res.update({"grad_" + k: x for k, x in zip(keys, g)})
    return res


def _check(got, ref, yard, what, names=BK.NAMES):
    """Prints yardstick, bound and error of every tensor, then asserts them together."""
    bad = []
    for n in names:
        if ref[n] is None or n not in yard:
            continue
        err, lim = BK.relerr(got[n], ref[n]), BK.bound(yard[n])
        print(f"{what} {n}: yardstick {yard[n]:.3g}, bound {lim:.3g}, error {err:.3g}")
        assert got[n].shape == ref[n].shape and got[n].dtype == torch.float32
        if not err <= lim:
            bad.append((n, err, lim))
    assert not bad, (what, bad)


@gpu
@pytest.mark.parametrize("regime", range(3))
@pytest.mark.parametrize("K", KS)
def test_constructed_planes_forward_and_all_four_gradients(K, regime):
    sigma, gamma = BK.REGIMES[regime]
    for D in DS:
        c = BK.constructed(K, D, sigma)
        ref, yard = BK.referee_and_yardstick(("constructed", K, D), c, sigma, gamma, "cuda")
        got = _fused(c, sigma, gamma)
        assert all(torch.isfinite(got[n]).all() for n in BK.NAMES)
        _check(got, ref, yard, f"K={K} D={D} sigma={sigma} gamma={gamma}")
        if K == 1 and gamma == 1e-4:
            # delta clamped, one fragment: the referee's z gradient is exactly 0; the derivative's analytic size bounds the kernel's
            assert "grad_zbuf" not in yard and not ref["grad_zbuf"].any()
            lim, worst = BK.kat_zbuf_limit(c, gamma), float(got["grad_zbuf"].abs().max())
            print(f"K=1 D={D} clamped delta: |grad_zbuf| {worst:.3g}, analytic limit {lim:.3g}")
            assert worst <= lim
        else:
            assert set(yard) == set(BK.NAMES)
        # empty pixels: the background colour and alpha 0, exactly; no gradient behind a pixel's fragments
        empty = torch.from_numpy(c["counts"] == 0).cuda()
        bg = torch.tensor(c["background"] + (0.0,), device="cuda")
        assert empty.sum() > 50 and torch.equal(got["out"][empty], bg.expand(int(empty.sum()), D + 1))
        pad = (c["pix_to_face"] < 0).cuda()
        assert not got["grad_zbuf"][pad].any() and not got["grad_dists"][pad].any() and not got["grad_bary"][pad].any()


@gpu
def test_saturated_layers_stay_finite_and_use_the_exclusive_product():
    sigma = gamma = 1e-4
    c = BK.saturated()
    ref, yard = BK.referee_and_yardstick("saturated", c, sigma, gamma, "cuda")
    got = _fused(c, sigma, gamma)
    assert all(torch.isfinite(got[n]).all() for n in BK.NAMES)
    _check(got, ref, yard, "saturated", names=("out", "grad_dists"))
    # the alpha-only form: the gradient of the product alone, against torch.prod's backward in float64
    p2f, go = c["pix_to_face"].cuda(), c["grad_out"][..., 3].cuda()
    d = c["dists"].cuda().requires_grad_(True)
    g_got, = torch.autograd.grad(blend_k_alpha(p2f, d, sigma), d, go)
    g = {}
    for dt in (torch.float64, torch.float32):
        dd = c["dists"].cuda().to(dt).requires_grad_(True)
        g[dt], = torch.autograd.grad(BK.torch_alpha(p2f, dd, sigma, dt), dd, go.to(dt))
    y = BK.relerr(g[torch.float32], g[torch.float64])
    err = BK.relerr(g_got, g[torch.float64])
    print(f"saturated alpha-only grad_dists: yardstick {y:.3g}, bound {BK.bound(y):.3g}, error {err:.3g}")
    assert torch.isfinite(g_got).all() and float(g[torch.float64].abs().max()) > 0 and err <= BK.bound(y)


@gpu
def test_everything_behind_the_first_negative_id_is_ignored():
    sigma, gamma = BK.REGIMES[1]
    c = BK.constructed(8, 3, sigma)
    clean = _fused(c, sigma, gamma)
    pad = c["pix_to_face"] < 0
    behind = pad & (torch.arange(8) > torch.from_numpy(c["counts"])[..., None])       # strictly behind the pixel's first -1
    assert int(pad.sum()) > 500 and int(behind.sum()) > 300
    dirty = dict(c)
    ids = c["pix_to_face"].clone()
    ids[behind] = torch.tensor([3, 10 ** 9, BK.N_FACES, -(10 ** 12)]).repeat(int(behind.sum()) // 4 + 1)[:int(behind.sum())]
    dirty["pix_to_face"] = ids
    for k in ("zbuf", "dists", "bary"):
        t = c[k].clone()
        t[pad] = float("nan")
        dirty[k] = t
    got = _fused(dirty, sigma, gamma)
    assert torch.equal(got["out"], clean["out"])
    for n in ("grad_zbuf", "grad_bary", "grad_dists"):
        assert torch.equal(got[n], clean[n]) and not got[n][pad.cuda()].any() and torch.isfinite(got[n]).all(), n
    assert torch.isfinite(got["grad_face_attr"]).all()
    y = BK.referee_and_yardstick(("constructed", 8, 3), c, sigma, gamma, "cuda")[1]["grad_face_attr"]
    assert BK.relerr(got["grad_face_attr"], clean["grad_face_attr"]) <= BK.bound(y)
    a_clean = blend_k_alpha(c["pix_to_face"].cuda(), c["dists"].cuda(), sigma)
    assert torch.equal(blend_k_alpha(ids.cuda(), dirty["dists"].cuda(), sigma), a_clean)


@gpu
@pytest.mark.parametrize("H,W", [(64, 64), (44, 77)])
def test_through_the_rasteriser_to_the_vertices(H, W):
    """ops.raster_k -> ops.blend_k -> backward against ops.raster_k -> the torch route in float64; both reach the vertices through the
    same foho_rastk_bwd, and the yardstick is the float32 torch route through it."""
    blur = 1e-3
    v, f = RK.two_spheres(H, W)
    df = torch.from_numpy(f).cuda()
    g = torch.Generator().manual_seed(3)
    attr = torch.randn(len(f), 3, 3, generator=g).cuda()
    bg = (0.2, 0.5, 0.9)
    for K in (4, 8):
        gout = torch.randn(H, W, 4, generator=g).cuda()
        for sigma, gamma in (BK.REGIMES[0], BK.REGIMES[2]):
            def vertex_grad(route):
                dv = torch.from_numpy(v).cuda().requires_grad_(True)
                p2f, z, b, d, _ = ops.raster_k(dv, df, H, W, K, blur)
                if route == "fused":
                    out = blend_k(p2f, z, b, d, attr, sigma, gamma, BK.ZNEAR, BK.ZFAR, bg)
                else:
                    out = BK.torch_route(dict(pix_to_face=p2f, zbuf=z, bary=b, dists=d), attr, bg, sigma, gamma, route)
                (out * gout.to(out.dtype)).sum().backward()
                assert ((p2f >= 0).sum(-1) >= 4).any() and ((p2f >= 0).sum(-1) == 0).any()      # the cut or near it, and pure padding
                return dict(out=out.detach(), grad_verts=dv.grad)
            ref, f32, got = vertex_grad(torch.float64), vertex_grad(torch.float32), vertex_grad("fused")
            yard = {n: BK.relerr(f32[n], ref[n]) for n in ref}
            assert torch.isfinite(got["grad_verts"]).all() and float(ref["grad_verts"].abs().max()) > 0
            _check(got, ref, yard, f"{H}x{W} K={K} sigma={sigma} gamma={gamma}", names=("out", "grad_verts"))


@gpu
def test_flags_unit_bary_and_alpha_only():
    sigma, gamma = BK.REGIMES[1]
    for K in (3, 100):
        c = BK.constructed(K, 3, sigma)
        ones = dict(c, bary=torch.ones_like(c["bary"]))
        a, b = _fused(c, sigma, gamma, unit_bary=True), _fused(ones, sigma, gamma)
        assert a["grad_bary"] is None and torch.equal(a["out"], b["out"])
        assert torch.equal(a["grad_zbuf"], b["grad_zbuf"]) and torch.equal(a["grad_dists"], b["grad_dists"])
        ref, yard = BK.referee_and_yardstick(("constructed", K, 3), c, sigma, gamma, "cuda", True)
        _check(a, ref, yard, f"unit_bary K={K}")
        alpha = blend_k_alpha(c["pix_to_face"].cuda(), c["dists"].cuda(), sigma)
        assert alpha.shape == BK.FRAME and torch.equal(alpha, _fused(c, sigma, gamma)["out"][..., 3]) and 0 < float(alpha.sum())


def _facade_scene(H, W, K, fused, sigma, gamma):
    from test_raster_k import _scene_mesh
    cams, verts, faces = _scene_mesh(H, W)
    rast = p3d.MeshRasterizer(cams, p3d.RasterizationSettings((H, W), 1e-3, K, k_fragments=True))
    return cams, verts, faces, rast, p3d.BlendParams(sigma, gamma, (0.3, 0.6, 0.9), fused=fused)


@gpu
@pytest.mark.parametrize("shader", ["phong", "silhouette"])
def test_facade_fused_against_unfused(shader, monkeypatch):
    H, W, K, sigma, gamma = 44, 77, 4, 1e-4, 1e-4
    gout = torch.randn(1, H, W, 4, generator=torch.Generator().manual_seed(9)).cuda()
    calls = []
    real = {n: getattr(ops, n) for n in ("blend_k", "blend_k_alpha")}
    for n in real:
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **kw: (calls.append(_n), real[_n](*a, **kw))[1])

    def render(route):
        cams, verts, faces, rast, bp = _facade_scene(H, W, K, route == "fused", sigma, gamma)
        mesh = p3d.Meshes([verts], [faces])
        if route == torch.float64:            # the referee: the shader's torch route in float64 on the float32 planes
            fr = rast(mesh)
            if shader == "phong":
                img = BK.torch_route(dict(pix_to_face=fr.pix_to_face[0], zbuf=fr.zbuf[0], bary=fr.bary_coords[0], dists=fr.dists[0]),
                                     mesh.verts_normals_packed()[faces], bp.background_color, sigma, gamma, route, True, cams.znear, cams.zfar)[None]
            else:
                a = BK.torch_alpha(fr.pix_to_face, fr.dists, sigma, route)
                img = torch.cat([torch.ones(a.shape + (3,), device="cuda", dtype=route), a[..., None]], -1)
            empty = None
        else:
            sh = (p3d.PhongNormalShader if shader == "phong" else p3d.SoftSilhouetteShader)(cameras=cams, blend_params=bp)
            img = p3d.MeshRenderer(rast, sh)(mesh)
            empty = (rast(mesh).pix_to_face[..., 0] < 0)
        (img * gout.to(img.dtype)).sum().backward()
        return dict(out=img.detach(), grad_verts=verts.grad), empty

    (ref, _), (plain, empty) = render(torch.float64), render(torch.float32)
    assert not calls                                          # fused=False: neither operator is called
    fused, _ = render("fused")
    assert calls == ["blend_k" if shader == "phong" else "blend_k_alpha"]
    yard = {n: BK.relerr(plain[n], ref[n]) for n in ref}
    assert fused["out"].shape == (1, H, W, 4) and fused["out"].dtype == torch.float32 and torch.isfinite(fused["grad_verts"]).all()
    assert float(plain["grad_verts"].abs().max()) > 0
    _check(fused, plain, yard, f"facade {shader} against fused=False", names=("out", "grad_verts"))
    _check(fused, ref, yard, f"facade {shader} against float64", names=("out", "grad_verts"))
    # empty pixels: the torch route's background colour and alpha 0, exactly
    assert empty.sum() > 500 and torch.equal(fused["out"][empty], plain["out"][empty])
    assert (fused["out"][empty][:, 3] == 0).all()
    if shader == "phong":
        assert torch.equal(fused["out"][empty][:, :3], torch.tensor((0.3, 0.6, 0.9), device="cuda").expand(int(empty.sum()), 3))


@gpu
def test_facade_blend_fragments_and_the_refusal_of_other_planes():
    H, W, K = 44, 77, 4
    cams, verts, faces, rast, bp = _facade_scene(H, W, K, True, 1e-4, 0.1)
    mesh = p3d.Meshes([verts], [faces])
    attr = torch.randn(len(faces), 3, 3, generator=torch.Generator().manual_seed(4)).cuda()
    fr = rast(mesh)
    assert fr.k_planes
    got = p3d.blend_fragments(fr, attr, bp, cams.znear, cams.zfar)
    planes = dict(pix_to_face=fr.pix_to_face[0], zbuf=fr.zbuf[0].detach(), bary=fr.bary_coords[0].detach(), dists=fr.dists[0].detach())
    ref = BK.torch_route(planes, attr, bp.background_color, bp.sigma, bp.gamma, torch.float64, False, cams.znear, cams.zfar)[None]
    plain = p3d.blend_fragments(fr, attr, p3d.BlendParams(bp.sigma, bp.gamma, bp.background_color), cams.znear, cams.zfar)
    y = BK.relerr(plain, ref)
    print(f"blend_fragments: yardstick {y:.3g}, bound {BK.bound(y):.3g}, error {BK.relerr(got, ref):.3g}")
    assert got.shape == (1, H, W, 4) and BK.relerr(got, ref) <= BK.bound(y)
    one = p3d.MeshRasterizer(cams, p3d.RasterizationSettings((H, W), 1e-3, K))(mesh)          # the default route: one fragment + sil_prod
    assert not one.k_planes
    for call in (lambda: p3d.PhongNormalShader(cameras=cams, blend_params=bp)(one, mesh), lambda: p3d.SoftSilhouetteShader(blend_params=bp)(one, mesh),
                 lambda: p3d.blend_fragments(one, attr, bp, cams.znear, cams.zfar)):
        with pytest.raises(ValueError, match="k_fragments=True"):
            call()


@gpu
def test_repeatable_bitwise_except_the_atomic_attribute_gradient():
    sigma, gamma = BK.REGIMES[0]
    c = BK.constructed(128, 4, sigma)
    a, b = _fused(c, sigma, gamma), _fused(c, sigma, gamma)
    for n in ("out", "grad_zbuf", "grad_bary", "grad_dists"):
        assert torch.equal(a[n], b[n]), n
    y = BK.referee_and_yardstick(("constructed", 128, 4), c, sigma, gamma, "cuda")[1]["grad_face_attr"]
    err = BK.relerr(a["grad_face_attr"], b["grad_face_attr"])
    print(f"grad_face_attr run to run: yardstick {y:.3g}, bound {BK.bound(y):.3g}, difference {err:.3g}")
    assert err <= BK.bound(y)


@gpu
def test_backward_computes_only_the_gradients_autograd_asks_for(monkeypatch):
    sigma, gamma = BK.REGIMES[1]
    c = BK.constructed(8, 3, sigma)
    full = _fused(c, sigma, gamma)
    L = _lib.rastk()
    real, seen = L.foho_rastk_blend_bwd, []

    def spy(*a):
        seen.append([x is not None and (x.value if isinstance(x, vp) else x) is not None for x in a[17:21]])
        return real(*a)

    monkeypatch.setattr(L, "foho_rastk_blend_bwd", spy)
    only = _fused(c, sigma, gamma, need=("dists",))
    assert seen == [[False, False, True, False]]
    assert torch.equal(only["grad_dists"], full["grad_dists"]) and only["grad_zbuf"] is None and only["grad_face_attr"] is None
    _fused(c, sigma, gamma)
    assert seen[1] == [True, True, True, True]
