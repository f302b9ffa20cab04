"""The FlexiCubes gradient (k_flexi_bwd: ops.flexicubes, engine.SdfObjective) against a float64 closed-form referee, over every cube case.

tests/flexi_grad_ref.py sums, per cube, patch and crossing edge, the four closed-form terms of d(dual vertex)/d(sdf, grid position) in
numpy.  Every comparison uses the rasteriser referee's measure, err = max |got - ref| / max(scale, 1e-4 scale.max()), with scale = the
sum of the magnitudes of the terms that land on a grid point (entry).

Fields: the ten fuzz fields of test_flexi.py (exact zeros, ties, several components, surfaces cut by the grid boundary; 241 of the 254
mixed sign codes, 83 of the 92 multi-patch ones) and `allcases` (res 16, every code 1..254 on a designated cube, 1278 multi-patch
cubes), both on a grid jittered by +-0.3 of a cell; `tiny` (3^3 points, D = 1e-30 on the crossing edges); `chain_multi` in two variants
(the chain tests' grid under a ripple: closed, 192 / 178 vertices, 18 / 10 multi-patch cubes).  Cotangents are seeded randn.

Tolerances.  TOL_F32 is the worst error of the referee's own float32 evaluation against its float64 one, over every field:
  measured  dL/ds 1.75e-6 (fuzz1; 1.26e-6 fuzz9, 7.2e-7 fuzz7, every other field 1.4e-7 .. 4.4e-7)   ->  TOL_F32 = 1.75e-6
            dL/dx 2.37e-7 (allcases; every other field 8.6e-8 .. 2.1e-7)                             ->  TOL_F32 = 2.4e-7
TOL, the kernels' bound, is 4 x TOL_F32 rounded up to one significant digit -- dL/ds 7e-6, dL/dx 1e-6: the kernel adds up to 24 terms
per grid point with float atomics in no fixed order, the referee adds them in one order.  Neither number comes from what the kernel
achieves; a kernel that needs more is a finding.  (The float32 autograd of the oracle, the yardstick before this file, is up to 9.7e-4
from float64 in this measure: cancellation in its quotient rule.)  The float64 referee against the oracle's float64 autograd -- two
independent derivations -- is within 2e-12 (bound 1e-10).

CPU: referee == float64 autograd, central differences, the conditions on the inputs, the float32 yardstick, corrupted referees that
must be caught.  GPU: ops.flexicubes with both gradients and with dL/ds alone, the shapes and dtypes ops.py promises, `tiny`, and the
iso-surface backward inside capacity mode (graph replay and eager) and on the exact-size path, each fed with the step's own vertex
gradient so that the step's float32 noise stays out of the comparison."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flexi_grad_ref as G  # noqa: E402
from oracle import flexi_ref as FR  # noqa: E402

gpu = pytest.mark.gpu
TOL_F32 = {"s": 1.75e-6, "x": 2.4e-7}      # the referee's own float32 evaluation against its float64 one (measured, see above)
TOL = {"s": 7e-6, "x": 1e-6}               # kernels against the referee: 4 x TOL_F32, rounded up to one significant digit
TOL_AUTOGRAD = 1e-10
WIDE = G.FUZZ + ("allcases",)              # the fields that go through ops.flexicubes with both gradients


def _errs(gs, gx, ref):
    return {"s": G.measure(gs, ref[0], ref[2])[0], "x": G.measure(gx, ref[1], ref[3])[0]}


def _topology(v, f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return np.unique(e, axis=0, return_counts=True)[1]


# ---------------------------------------------------------------- CPU
def test_tolerances_follow_from_the_yardstick():
    for k in ("s", "x"):
        lead = 10.0 ** np.floor(np.log10(4 * TOL_F32[k]))
        assert TOL[k] == pytest.approx(np.ceil(4 * TOL_F32[k] / lead - 1e-9) * lead, rel=1e-12)


def test_inputs_reach_what_they_were_built_for():
    """Conditions on the fields (if one breaks, change the seed, never the condition)."""
    c = G.case("allcases")
    code = c.code.reshape(16, 16, 16)
    want = np.array([[[G.allcases_code(a, b, cc) for cc in range(8)] for b in range(8)] for a in range(8)])
    assert np.array_equal(code[::2, ::2, ::2], want) and set(want.reshape(-1).tolist()) == set(range(1, 255))
    multi, mixed = set(), set()
    for name in G.FUZZ:
        f = G.case(name)
        assert f.nv > 20
        mixed |= set(f.code.tolist())
        multi |= set(f.code[G.N_PATCH[f.code] > 1].tolist())
    mixed -= {0, 255}
    print(f"fuzz fields: {len(mixed)} of 254 mixed codes, {len(multi)} of {len(G.MULTI_CODES)} multi-patch codes; "
          f"allcases: {c.nv} vertices, {c.n_multi()} multi-patch cubes")
    assert len(G.MULTI_CODES) == 92 and len(multi) >= 80
    sizes = set()
    for name in G.CHAIN:
        f = G.case(name)
        V, F, _ = FR.flexicubes(f.x, f.s, f.res)
        print(f"{name}: {len(V)} vertices, {len(F)} faces, {f.n_multi()} multi-patch cubes")
        assert len(V) == f.nv and (_topology(V.numpy(), F.numpy()) == 2).all()      # closed: every edge shared by two faces
        assert f.n_multi() >= 10
        sizes.add(f.nv)
    assert len(sizes) == len(G.CHAIN)
    t = G.case("tiny")
    assert t.nv == 8 and float(t.ref[0].abs().max()) < 3e38 and bool(torch.isfinite(t.ref[0]).all())
    # D * D is zero in float32 on tiny's crossing edges: the form 1 / (D * D) cannot evaluate it
    assert np.float32(1e-30) * np.float32(1e-30) == 0


@pytest.mark.parametrize("name", [n for n in G.FIELDS if n != "tiny"])
def test_referee_equals_float64_autograd_of_the_oracle(name):
    """Two independent derivations: the closed form and torch autograd through oracle.flexi_ref.flexicubes, both in float64."""
    c = G.case(name)
    xd, sd = c.x.double().requires_grad_(True), c.s.double().requires_grad_(True)
    V, _, _ = FR.flexicubes(xd, sd, c.res)
    (V * c.gv.double()).sum().backward()
    e = _errs(sd.grad, xd.grad, c.ref)
    print(f"{name}: referee against float64 autograd  dL/ds {e['s']:.2e}  dL/dx {e['x']:.2e}")
    assert e["s"] <= TOL_AUTOGRAD and e["x"] <= TOL_AUTOGRAD, e


def test_referee_matches_central_differences_on_allcases():
    """Spot check in float64, h = 1e-5: truncation h^2/6 |f'''| <= 1e-8 scale (D >= 0.1 on allcases), rounding 2.2e-16 |L| / h ~ 1e-8;
    bound 1e-6 of max(scale, 1)."""
    c = G.case("allcases")
    x, s, w, h = c.x.double(), c.s.double(), c.gv.double(), 1e-5
    L = lambda xx, ss: float((FR.flexicubes(xx, ss, c.res)[0] * w).sum())
    gs, gx, ss_, sx_ = c.ref
    multi_pts = set()
    for cube in np.flatnonzero(G.N_PATCH[c.code] > 1):
        i, j, k = np.unravel_index(cube, (16, 16, 16))
        multi_pts |= {((i + a) * 17 + (j + b)) * 17 + (k + d) for a, b, d in FR.CORNERS}
    live = [int(i) for i in torch.nonzero(ss_).reshape(-1) if int(i) in multi_pts]
    assert len(live) > 1000
    worst = 0.0
    for n, i in enumerate(live[::len(live) // 8][:8]):
        sp, sm = s.clone(), s.clone()
        sp[i] += h
        sm[i] -= h
        e = abs((L(x, sp) - L(x, sm)) / (2 * h) - float(gs[i])) / max(float(ss_[i]), 1.0)
        xp, xm = x.clone(), x.clone()
        xp[i, n % 3] += h
        xm[i, n % 3] -= h
        e2 = abs((L(xp, s) - L(xm, s)) / (2 * h) - float(gx[i, n % 3])) / max(float(sx_[i, n % 3]), 1.0)
        worst = max(worst, e, e2)
        assert e <= 1e-6 and e2 <= 1e-6, (i, e, e2)
    print(f"allcases: central differences at 8 grid points of multi-patch cubes, worst {worst:.2e}")


def test_float32_yardstick():
    """The referee evaluated in float32 against itself in float64, per field: what float32 arithmetic achieves on this formula.
    Its worst value is TOL_F32 (a field that exceeds it means the header's figures are stale, not that the bound may grow unseen)."""
    worst = {"s": 0.0, "x": 0.0}
    for name in G.FIELDS:
        c = G.case(name)
        r32 = G.grad(c.x.numpy(), c.s.numpy(), c.res, c.gv.numpy(), dtype=np.float32)
        assert bool(torch.isfinite(r32[0]).all()) and bool(torch.isfinite(r32[1]).all())
        e = _errs(r32[0], r32[1], c.ref)
        print(f"{name}: float32 referee against float64  dL/ds {e['s']:.3e}  dL/dx {e['x']:.3e}")
        worst = {k: max(worst[k], e[k]) for k in worst}
    print(f"worst: dL/ds {worst['s']:.3e} (TOL_F32 {TOL_F32['s']:.2e}, TOL {TOL['s']:.0e})  "
          f"dL/dx {worst['x']:.3e} (TOL_F32 {TOL_F32['x']:.2e}, TOL {TOL['x']:.0e})")
    for k in worst:
        assert 0.9 * TOL_F32[k] <= worst[k] <= TOL_F32[k], (k, worst[k])


def test_corrupted_referees_are_caught():
    """Teeth: each wrong formula is more than 100 x TOL from the referee on allcases.  And the gap this file closes: dropping the
    patches p >= 1 is invisible -- error exactly 0 -- on the four smooth fields test_flexi.py takes its gradient on."""
    c = G.case("allcases")
    for cor in G.CORRUPTIONS:
        r = G.grad(c.x.numpy(), c.s.numpy(), c.res, c.gv.numpy(), corrupt=cor)
        e = _errs(r[0], r[1], c.ref)
        print(f"allcases, {cor}: dL/ds {e['s']:.3e}  dL/dx {e['x']:.3e}")
        assert e["s"] > 100 * TOL["s"]
        if cor != "swap_gs":                                   # swapping the two dL/ds terms leaves dL/dx alone
            assert e["x"] > 100 * TOL["x"]
    for name in G.SMOOTH:
        f = G.case(name)
        r = G.grad(f.x.numpy(), f.s.numpy(), f.res, f.gv.numpy(), corrupt="drop_patches")
        e = _errs(r[0], r[1], f.ref)
        print(f"{name} (res {f.res}, {f.nv} vertices, {f.n_multi()} multi-patch cubes), drop_patches: dL/ds {e['s']}  dL/dx {e['x']}")
        assert f.n_multi() == 0 and e["s"] == 0.0 and e["x"] == 0.0


# ---------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("name", WIDE)
def test_hip_gradients_match_the_referee(name):
    """ops.flexicubes with x and s requiring grad on a jittered grid: the forward stays bit-equal to the oracle, dL/ds and dL/dx are
    within TOL of the referee, grid points no crossing edge ends at get exact zeros; with s alone requiring grad, x.grad stays None."""
    from followmyhold_amd import ops
    c = G.case(name)
    V, F, _ = FR.flexicubes(c.x, c.s, c.res)
    xg, sg = c.x.cuda().requires_grad_(True), c.s.cuda().requires_grad_(True)
    v, f, _ = ops.flexicubes(xg, sg, c.res)
    assert torch.equal(f.cpu(), F) and torch.equal(v.detach().cpu(), V)
    (v * c.gv.cuda()).sum().backward()
    e = _errs(sg.grad, xg.grad, c.ref)
    s1 = c.s.cuda().requires_grad_(True)
    x1 = c.x.cuda()
    v1, _, _ = ops.flexicubes(x1, s1, c.res)
    (v1 * c.gv.cuda()).sum().backward()
    e1 = G.measure(s1.grad, c.ref[0], c.ref[2])[0]
    print(f"{name}: dL/ds {e['s']:.3e} (alone {e1:.3e}, TOL {TOL['s']:.0e})  dL/dx {e['x']:.3e} (TOL {TOL['x']:.0e})")
    assert e["s"] <= TOL["s"] and e["x"] <= TOL["x"], e
    assert not bool(sg.grad.cpu()[c.ref[2] == 0].any()) and not bool(xg.grad.cpu()[c.ref[3] == 0].any())
    assert x1.grad is None and e1 <= TOL["s"], e1


@gpu
@pytest.mark.parametrize("name", ["fuzz0", "allcases"])
def test_hip_gradients_keep_shape_and_dtype(name):
    """A (G,G,G) half-precision SDF gets a (G,G,G) half-precision gradient, within 2^-10 (half a unit of fp16 and TOL) of the referee on
    the fp16-rounded values; float64 grid positions get a float64 gradient of their own shape within TOL."""
    from followmyhold_amd import ops
    c = G.case(name)
    Gn = c.res + 1
    sh = c.s.half()
    nv = G.n_verts(sh.float().numpy(), c.res)
    gv = G.cotangent(nv, seed=12)
    ref = G.grad(c.x.numpy(), sh.float().numpy(), c.res, gv.numpy())
    assert float(ref[0].abs().max()) < 6e4                     # representable in fp16
    s3 = sh.reshape(Gn, Gn, Gn).cuda().requires_grad_(True)
    xd = c.x.double().cuda().requires_grad_(True)
    v, _, _ = ops.flexicubes(xd, s3, c.res)
    assert len(v) == nv
    (v * gv.cuda()).sum().backward()
    assert s3.grad.shape == (Gn, Gn, Gn) and s3.grad.dtype == torch.float16
    assert xd.grad.shape == (Gn ** 3, 3) and xd.grad.dtype == torch.float64
    es = G.measure(s3.grad.reshape(-1), ref[0], ref[2])[0]
    ex = G.measure(xd.grad, ref[1], ref[3])[0]
    print(f"{name}: fp16 dL/ds {es:.3e} (bound {2.0 ** -10:.3e})  float64-typed dL/dx {ex:.3e} (TOL {TOL['x']:.0e})")
    assert es <= 2.0 ** -10 and ex <= TOL["x"]


@gpu
def test_hip_gradient_is_finite_where_d_squared_underflows():
    """`tiny`: D = 1e-30 on the six crossing grid edges, the gradient reaches 1e30 and fits float32.  1 / (D * D) gave six infinities
    and a NaN; the kernel divides twice, (s / D) / D, which overflows only where the value does."""
    from followmyhold_amd import ops
    c = G.case("tiny")
    xg, sg = c.x.cuda().requires_grad_(True), c.s.cuda().requires_grad_(True)
    v, f, _ = ops.flexicubes(xg, sg, c.res)
    V, F, _ = FR.flexicubes(c.x, c.s, c.res)
    assert torch.equal(f.cpu(), F) and torch.equal(v.detach().cpu(), V) and len(v) == 8
    (v * c.gv.cuda()).sum().backward()
    gs, gx = sg.grad.cpu(), xg.grad.cpu()
    print(f"tiny: dL/ds {gs.tolist()}  largest reference {float(c.ref[0].abs().max()):.3e}")
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gx).all())
    e = _errs(gs, gx, c.ref)
    print(f"tiny: dL/ds {e['s']:.3e}  dL/dx {e['x']:.3e}")
    assert e["s"] <= TOL["s"] and e["x"] <= TOL["x"], e


@gpu
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_capacity_mode_backward_matches_the_referee(use_graph):
    """engine.SdfObjective, B = 2, one chain_multi variant per image: foho_flexi_bwd with n_verts = the capacity, per image, inside the
    captured chain.  The referee is fed each image's own vertex gradient as the step left it, so only the iso-surface backward is
    compared; the rows that carry a gradient are exactly the end points of crossing edges."""
    from followmyhold_amd import engine as E
    _, sc0, x, _ = G.chain_scene(0)
    _, sc1, _, _ = G.chain_scene(5)
    cases = [G.case(n) for n in G.CHAIN]
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    gb = E.GuidanceBatch([sc0, sc1], grid_res=16, obj_capacity=(2048, 4096))
    o = E.SdfObjective(gb, x, G.CHAIN_RES)
    o.run(torch.stack([c.s for c in cases]).cuda(), cfg, use_graph=use_graph)
    torch.cuda.synchronize()
    st, rows = o.status(), o.active_rows()
    for b, c in enumerate(cases):
        nv, nf, flags = st[b]
        assert flags == 0 and nv == c.nv
        lo, _ = gb.obj_slot(b)
        gv = gb.grad_verts_in[lo:lo + nv].cpu()
        assert float(gv.abs().max()) > 0
        ref = G.grad(c.x.numpy(), c.s.numpy(), c.res, gv.numpy())
        e = G.measure(o.grad_sdf[b], ref[0], ref[2])[0]
        print(f"image {b} ({c.name}, {nv} vertices, {'graph' if use_graph else 'eager'}): dL/ds {e:.3e} (TOL {TOL['s']:.0e}), "
              f"{rows[b]} active rows")
        assert e <= TOL["s"], e
        assert rows[b] == int((ref[2] > 0).sum())


@gpu
@pytest.mark.parametrize("name", G.CHAIN)
def test_exact_size_chain_backward_matches_the_referee(name):
    """ops.flexicubes -> gb.objective: the vertex gradient the step hands back (v.grad) through the referee against s.grad."""
    from followmyhold_amd import engine as E, ops
    _, npsc, x, _ = G.chain_scene(0)
    c = G.case(name)
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    gb = E.GuidanceBatch([npsc], grid_res=16)
    sg = c.s.cuda().requires_grad_(True)
    v, f, _ = ops.flexicubes(x.cuda(), sg, c.res)
    v.retain_grad()
    gb.objective(v, f, cfg).backward()
    torch.cuda.synchronize()
    gb.raise_on_flags()
    assert len(v) == c.nv
    ref = G.grad(c.x.numpy(), c.s.numpy(), c.res, v.grad.cpu().numpy())
    e = G.measure(sg.grad, ref[0], ref[2])[0]
    print(f"{name}: exact-size chain dL/ds {e:.3e} (TOL {TOL['s']:.0e})")
    assert e <= TOL["s"], e
    assert int(torch.count_nonzero(sg.grad)) == int((ref[2] > 0).sum())
