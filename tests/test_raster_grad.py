"""The rasteriser gradients (ops.raster_bwd, ops.raster_k_bwd, ops.raster_k, the facade) against a float64 per-fragment referee.

tests/raster_grad_ref.py differentiates oracle.ref_ops' fragment arithmetic in float64, one copy of the face per fragment.  Every
comparison uses one measure, err = max |got - ref| / max(scale, 1e-4 scale.max()) with scale = the sum of the fragments' gradient
magnitudes at the vertex, and one tolerance for the kernels, 1e-4: the gradient parity foho_common.h states for its reciprocal-based
gradient arithmetic (fdiv).  Fragments next to a kink (a barycentric near 0, two nearly equal edge distances) are taken out on both
sides by zeroing their incoming gradients; at most 2 % of a scene's fragments may go that way.

Scenes: the two spheres without their sub-pixel slivers, blurred by a pixel so that most fragments lie OUTSIDE their face (the clamp
branches of eval_frag_bwd); six faces cut by the near plane, one and two vertices behind under all three rotations, at the reference
blur and at a pixel's.  CPU: the referee reproduces the forward planes, the guard's share, its float32 evaluation, central
differences, and corrupted referees that must be caught.  GPU: each incoming plane alone and all together, for every scene, frame
and K."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_grad_ref as G  # noqa: E402
import rastk_ref as RK  # noqa: E402
from oracle import clib  # noqa: E402

gpu = pytest.mark.gpu
TOL = 1e-4             # kernels against the referee (foho_common.h: "parity there is 1e-4 relative")
TOL_F32 = 1e-5         # the referee's own float32 evaluation against its float64 one
GUARD_CAP = 0.02
PLANES = ("z", "bary", "dists", "all")


def _blur(kind, H, W):
    return RK.BLUR if kind == "ref" else (2.0 / min(H, W)) ** 2


# (scene, H, W, blur, K, cull)
SPHERES = [("spheres", H, W, "pixel", K, False) for H, W in ((64, 64), (44, 77)) for K in (1, 3, 4, 8)]
SPHERES += [("spheres", 44, 77, "pixel", 100, False), ("spheres", 64, 64, "pixel", 4, True)]
SIX = [("six", H, W, b, K, False) for H, W in ((96, 96), (40, 56)) for b in ("ref", "pixel") for K in (1, 3, 4, 8)]
CASES = SPHERES + SIX
DEEP = [c for c in CASES if c[4] == 8 or c[4] == 100 or c[5]]          # one K per scene, frame and blur for the costlier CPU tests
_id = lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-K{c[4]}" + ("-cull" if c[5] else "")


class Case:
    """One scene rasterised by the oracle, its referee, the incoming gradients (guarded fragments zeroed) and the float64 reference
    of each plane; computed once and shared by every test that names the case."""

    def __init__(self, scene, H, W, blur, K, cull):
        self.name, self.H, self.W, self.K, self.cull = _id((scene, H, W, blur, K, cull)), H, W, K, cull
        self.blur = _blur(blur, H, W)
        self.v, self.f = G.pruned_spheres(H, W) if scene == "spheres" else G.six_clipped_faces()
        self.planes = RK.oracle("grad_" + scene, self.v, self.f, H, W, self.blur, K, cull=cull)
        self.ref = G.Referee(self.v, self.f, *self.planes, clib.get_z_clip())
        g = torch.Generator().manual_seed(5)
        m = self.ref.keep_mask()
        gz, gb, gd = torch.randn(H, W, K, generator=g) * m, torch.randn(H, W, K, 3, generator=g) * m[..., None], torch.randn(H, W, K, generator=g) * m
        self.incoming = dict(z=(gz, None, None), bary=(None, gb, None), dists=(None, None, gd), all=(gz, gb, gd))

    @functools.lru_cache(maxsize=None)
    def reference(self, plane):
        ref, scale, _ = self.ref.grad(*self.incoming[plane])
        assert float(ref.abs().max()) > 0
        return ref, scale


@functools.lru_cache(maxsize=None)
def case(*key):
    return Case(*key)


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("key", CASES, ids=_id)
def test_referee_reproduces_the_forward_and_the_guard_stays_under_its_cap(key):
    """Before anything is differentiated: the float64 referee, with its own choice of the half of a clipped face, gives the oracle's
    depth and (unclipped-face) barycentrics to 1e-5 and its distances to 1e-5 absolute or relative; the guard removes at most 2 % of
    the fragments (change the seed of a scene that breaks the cap, never the cap); and the scene reaches what it was built for."""
    c = case(*key)
    r = c.ref
    share = float((~r.keep).float().mean())
    print(f"{c.name}: {len(c.f)} faces, {len(r.frag)} fragments, {int(r.outside.sum())} outside their face, {int(r.strad.sum())} on clipped "
          f"faces ({int(r.second.sum())} from the second half), forward error {r.fwd_err}, guarded {share:.4f}")
    assert r.fwd_err["z"] <= 1e-5 and r.fwd_err["bary"] <= 1e-5 and r.fwd_err["dists"] <= 1e-5, r.fwd_err
    assert share <= GUARD_CAP, share
    if key[0] == "spheres":
        assert len(r.frag) > 200 and int(r.outside.sum()) > len(r.frag) // 2 and not bool(r.strad.any())
        if key[4] >= 3 and not key[5]:
            assert int(RK.tie_pixels(c.planes[0], c.planes[1]).sum()) == 0 and (c.planes[0] >= 0).sum(-1).max() >= 3
    else:
        faces = torch.from_numpy(c.planes[0]).reshape(-1)[r.frag]
        assert bool(r.second.any()) and not bool(r.second[r.strad].all()) and int(r.strad.sum()) > 100
        if key[4] >= 4:                                 # every layer is kept, so each face shows all it has
            for f in range(6):                          # face 2j + c: rotation j of the one-behind (c = 0) / two-behind (c = 1) face
                assert int((faces == f).sum()) > 10, f
            for f in (0, 2, 4):
                assert bool(r.second[faces == f].any()) and not bool(r.second[faces == f].all()), f
        if key[3] == "pixel" and key[4] >= 4:
            assert int((r.outside & r.strad).sum()) > 100


@pytest.mark.parametrize("key", DEEP, ids=_id)
def test_float32_evaluation_of_the_referee_is_the_yardstick(key):
    """What plain float32 arithmetic of the same formulas gives against float64, in the measure the kernels are held to: 1e-5 at the
    most on the kept fragments, a tenth of the kernels' tolerance.  (With the sub-pixel slivers left in, it is 5e-3.)"""
    c = case(*key)
    for plane in PLANES:
        ref, scale = c.reference(plane)
        r32, _, _ = c.ref.grad(*c.incoming[plane], dtype=torch.float32)
        err, _ = G.measure(r32, ref, scale)
        print(f"float32 referee {c.name} {plane}: {err:.3g}")
        assert err <= TOL_F32, (plane, err)


def test_central_differences_of_the_referee_on_the_clipped_faces():
    """Float64 central differences of depth, face barycentrics and distance of a dozen fragments of the six-face scene (two of each
    face: both halves, inside and outside) against the referee's autograd gradient, per fragment and plane."""
    c = case("six", 96, 96, "pixel", 8, False)
    r = c.ref
    faces = torch.from_numpy(c.planes[0]).reshape(-1)[r.frag]
    pick = []
    for f in range(6):
        ok = ((faces == f) & (r.margin > 0.05)).nonzero(as_tuple=True)[0]
        out = ok[r.outside[ok]]
        sec = ok[r.second[ok]] if f % 2 == 0 else ok[~r.outside[ok]]
        assert len(out) and len(sec), f
        pick += [int(out[len(out) // 2]), int(sec[len(sec) // 2])]
    p2f = np.full_like(c.planes[0], -1).reshape(-1)
    sel = r.frag[torch.tensor(sorted(set(pick)))].numpy()
    p2f[sel] = c.planes[0].reshape(-1)[sel]
    small = G.Referee(c.v, c.f, p2f.reshape(c.planes[0].shape), *c.planes[1:], clib.get_z_clip())
    n = len(small.frag)
    assert n == 12 and bool(small.second.any()) and bool(small.outside.any()) and not bool(small.outside.all())
    gen = torch.Generator().manual_seed(3)
    weights = dict(z=torch.randn(n, generator=gen, dtype=torch.float64), bary=torch.randn(n, 3, generator=gen, dtype=torch.float64),
                   dists=torch.randn(n, generator=gen, dtype=torch.float64))
    base = small.verts.double()[small.fidx]
    for i, plane in enumerate(("z", "bary", "dists")):
        def fn(fv):                                     # one value per fragment: the rows are independent
            out = small.planes(fv)[i] * weights[plane]
            return out.sum(1) if out.dim() == 2 else out
        fv = base.clone().requires_grad_(True)
        g, = torch.autograd.grad(fn(fv).sum(), fv)
        worst = 0.0
        for k in range(3):
            for q in range(3):
                h = 1e-7 * base[:, k, q].abs().clamp(min=1e-2)
                fp, fm = base.clone(), base.clone()
                fp[:, k, q] += h
                fm[:, k, q] -= h
                with torch.no_grad():
                    fd = (fn(fp) - fn(fm)) / (2 * h)
                worst = max(worst, float(((fd - g[:, k, q]).abs() / g.abs().reshape(n, -1).max(1).values).max()))
        print(f"central differences, {plane}: {worst:.3g} of the fragment's largest component")
        assert float(g.abs().max()) > 0 and worst <= 1e-6, (plane, worst)


def test_corrupted_referees_are_caught():
    """Teeth: each wrong derivative must exceed the kernels' tolerance by at least 100x on the plane it spoils.
    (a) the barycentric gradient taken w.r.t. the sub-triangle's barycentrics (what the kernels did before they converted it),
    (b) the crossing weights w2, w3 held constant, both on the clipped faces;
    (c) the area's derivative dropped: it is NOT caught, and cannot be -- the perspective barycentrics t_i / sum t are homogeneous of
        degree 0 in the area, so its exact derivative is zero wherever the sum is above its floor; the test pins that (1e-12), and two
        wrong terms that do matter take its place where fragments lie outside their face: the w >= 0 mask of the clamp dropped (z
        and barycentric planes), and the inside sign of the distance dropped."""
    six = [case("six", 96, 96, b, 8, False) for b in ("ref", "pixel")]
    sph = [case("spheres", 64, 64, "pixel", 8, False), case("spheres", 44, 77, "pixel", 8, False)]

    def err(c, plane, variant):
        ref, scale = c.reference(plane)
        e = G.measure(c.ref.grad(*c.incoming[plane], variant=variant)[0], ref, scale)[0]
        print(f"corrupted referee {variant} {c.name} {plane}: {e:.3g}")
        return e

    for c in six:
        for variant in ("sub_bary", "detach_w"):
            for plane in ("bary", "all"):
                assert err(c, plane, variant) >= 100 * TOL
            assert err(c, "z", variant) == 0 and err(c, "dists", variant) == 0          # and only there
    for c in six + sph:
        for plane in PLANES:
            assert err(c, plane, "no_area") <= 1e-12
        if c is not six[0]:                             # the reference blur leaves next to no fragment outside its face
            for plane in ("z", "bary", "all"):
                assert err(c, plane, "no_mask") >= 100 * TOL
        assert err(c, "dists", "no_flip") >= 100 * TOL


# ---------------------------------------------------------------- GPU
def _dev(c):
    return torch.from_numpy(c.v).cuda(), torch.from_numpy(c.f).cuda()


def _cuda(t):
    return None if t is None else t.cuda()


def _check(c, op, run):
    """run(gz, gb, gd) -> (V,3) on each plane alone and on all three; prints every error, then asserts them."""
    errs = {}
    for plane in PLANES:
        ref, scale = c.reference(plane)
        got = run(*(_cuda(t) for t in c.incoming[plane]))
        assert got.shape == ref.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        errs[plane], at = G.measure(got, ref, scale)
        print(f"{op} {c.name} {plane}: error {errs[plane]:.3g} (vertex {at // 3}, component {at % 3}; largest gradient {float(ref.abs().max()):.3g})")
    assert all(e <= TOL for e in errs.values()), errs


@gpu
@pytest.mark.parametrize("key", CASES, ids=_id)
def test_raster_k_bwd_against_the_referee(key):
    from followmyhold_amd import ops
    c = case(*key)
    dv, df = _dev(c)
    p2f = torch.from_numpy(c.planes[0]).cuda()
    _check(c, "raster_k_bwd", lambda gz, gb, gd: ops.raster_k_bwd(dv, df, p2f, gz, gb, gd, blur_radius=c.blur))


@gpu
@pytest.mark.parametrize("key", [k for k in CASES if k[4] == 1], ids=_id)
def test_raster_bwd_against_the_referee(key):
    from followmyhold_amd import ops
    c = case(*key)
    dv, df = _dev(c)
    p2f = torch.from_numpy(c.planes[0][..., 0].copy()).cuda()
    one = lambda t: None if t is None else t[:, :, 0].contiguous()
    _check(c, "raster_bwd", lambda gz, gb, gd: ops.raster_bwd(dv, df, p2f, one(gz), one(gb), one(gd), blur_radius=c.blur))


@gpu
def test_raster_k_end_to_end_against_the_referee():
    """ops.raster_k(...).backward(): the forward's own pix_to_face (the oracle's, asserted) and autograd's hand-over of the gradients."""
    from followmyhold_amd import ops
    c = case("six", 40, 56, "ref", 4, False)
    dv, df = _dev(c)

    def run(gz, gb, gd):
        v = dv.clone().requires_grad_(True)
        p2f, z, b, d, _ = ops.raster_k(v, df, c.H, c.W, c.K, c.blur)
        assert np.array_equal(p2f.cpu().numpy(), c.planes[0])
        loss = sum((a * g).sum() for a, g in ((z, gz), (b, gb), (d, gd)) if g is not None)
        loss.backward()
        return v.grad

    _check(c, "raster_k autograd", run)


class _NdcCamera:
    """The scenes hold NDC vertices already: a camera whose NDC transform is the identity."""
    znear, zfar = 0.01, 100.0

    def transform_points_ndc(self, pts):
        return pts


@gpu
@pytest.mark.parametrize("k_fragments", [False, True])
def test_facade_bary_gradient_on_the_clipped_faces(k_fragments):
    """MeshRasterizer at K = 1 (ops.raster_fwd / raster_bwd) and with k_fragments=True (ops.raster_k), then
    interpolate_face_attributes: a loss linear in bary_coords and one linear in the interpolated attributes."""
    from followmyhold_amd import facade as p3d
    K = 4 if k_fragments else 1
    c = case("six", 40, 56, "ref", K, False)
    dv, df = _dev(c)
    ref, scale = c.reference("bary")
    gb = c.incoming["bary"][1].cuda()
    rast = p3d.MeshRasterizer(_NdcCamera(), p3d.RasterizationSettings((c.H, c.W), c.blur, K, k_fragments=k_fragments))
    v = dv.clone().requires_grad_(True)
    frag = rast(p3d.Meshes([v], [df]))
    assert np.array_equal(frag.pix_to_face[0].cpu().numpy(), c.planes[0])
    assert float((frag.bary_coords[0].detach().cpu() - torch.from_numpy(c.planes[2])).abs().max()) <= 1e-6
    (frag.bary_coords[0] * gb).sum().backward()
    err, _ = G.measure(v.grad, ref, scale)
    print(f"facade k_fragments={k_fragments} {c.name} bary: error {err:.3g}")
    assert err <= TOL, err
    # the same through interpolate_face_attributes: sum_k bary_k attr[face, k] . weight  =  bary . (attr[face] . weight)
    gen = torch.Generator().manual_seed(9)
    attr = torch.randn(len(c.f), 3, 2, generator=gen).cuda()
    wgt = torch.randn(c.H, c.W, K, 2, generator=gen).cuda() * c.ref.keep_mask().cuda()[..., None]
    v2 = dv.clone().requires_grad_(True)
    frag = rast(p3d.Meshes([v2], [df]))
    (p3d.interpolate_face_attributes(frag.pix_to_face, frag.bary_coords, attr)[0] * wgt).sum().backward()
    gb2 = (attr[frag.pix_to_face[0].clamp(min=0)] * wgt[..., None, :]).sum(-1) * (frag.pix_to_face[0] >= 0)[..., None]
    ref2, scale2, _ = c.ref.grad(None, gb2.cpu(), None)
    err2, _ = G.measure(v2.grad, ref2, scale2)
    print(f"facade k_fragments={k_fragments} {c.name} interpolated attributes: error {err2:.3g}")
    assert err2 <= TOL, err2
