"""The weighted FlexiCubes (ops.flexicubes_weighted, facade.FlexiCubes with weights or training=True; libfoho_wflexi.so) against the
torch referee of tests/wflexi_ref.py, forward and all five gradients, in both modes.

Fields: flexi_grad_ref's ten fuzz fields (exact zeros, ties, surfaces cut by the grid boundary), `allcases` (res 16, every sign code,
jittered grid) and `tiny` (D = 1e-30 on the crossing edges).  Weights (wflexi_ref.weights, seeded per field): alpha and beta uniform
in the façade's reachable range (0.01, 1.99), gamma on eight levels inside (0.005, 0.995) whose pairwise products are exact in float32,
so exact ties of the two diagonal products occur and near-ties do not; on `allcases` and `fuzz1` also one set with every weight at an
end of its range.  Cotangents: seeded randn on all vertices (centres included) and on l_dev.

Where every crossing of a patch falls on one point -- a patch around a corner whose neighbours are exact zeros of the field, 1339 dual
vertices of the fuzz fields -- l_dev is the norm at 0: its gradient is defined as 0, and what any floating-point evaluation computes there
is the direction of a rounding error.  The l_dev cotangent is zero on those vertices (largest d_e under 1e-6 of a cell in the float64
referee); their vertex cotangent stays.

Error measure: flexi_grad_ref.measure, err = max |got - ref| / max(scale, 1e-4 scale.max()), with the referee's scale arrays (the sums
of the magnitudes of the terms that land on an entry; for the forward values the magnitudes of the crossings' terms).

Tolerances.  TOL_F32 is the worst error of the referee's own float32 evaluation against its float64 one over every case and both modes,
measured on the CPU (the field that sets each):
  vertices and centres  3.856e-7  (allcases, ends, training)      l_dev  9.531e-8  (allcases)
  dL/ds      3.787e-5  (fuzz1, ends)               dL/dx     2.658e-4  (fuzz6, training)
  dL/dalpha  9.117e-3  (fuzz1, ends)               dL/dbeta  8.173e-3  (fuzz7)              dL/dgamma  6.643e-3  (fuzz7)
(every other case: vertices 1.1e-7 .. 3.3e-7, l_dev 4.1e-8 .. 8.2e-8, dL/ds 3.8e-7 .. 3.4e-5, dL/dx 1.3e-7 .. 1.4e-4, dL/dalpha up to
3.9e-3, dL/dbeta 2.0e-6 .. 7.6e-3, dL/dgamma 2.7e-7 .. 4.5e-3.)  With a cotangent on the vertices alone dL/ds and dL/dx stay under 4e-7:
what lifts them is l_dev's (z_e - v) / d_e where d_e is a small fraction of a cell, a difference of two nearby points.
dL/dalpha, dL/dbeta and dL/dgamma are large next to the others because a copy holds ONE term -- g . (x_a - x_b) w / D^2 s,
g . (u_e - v) / B, g . (m - centre) gamma / den -- whose own dot product cancels: the scale is the term's magnitude, not its addends'.
TOL, the kernels' bound, is 4 x TOL_F32 rounded up to one significant digit: the project's margin for "another order of summation"
(test_flexi_grad.py).  None of these numbers is taken from what the kernels achieve; a kernel that needs more is a finding.

CPU: unit weights equal the oracle, the conditions on the inputs, central differences, the yardstick, corrupted referees, the C ABI of
libfoho_wflexi.so and its argument checks.  GPU: unit weights equal ops.flexicubes bitwise, the weighted forward and gradients in both
modes, `tiny`, repeatability, capacity overflow, the façade (forward, training, end to end) and the error paths."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flexi_grad_ref as G  # noqa: E402
import wflexi_ref as W  # noqa: E402
from oracle import flexi_ref as FR  # noqa: E402
from followmyhold_amd import _lib, weighted_flexi as WF  # noqa: E402
from followmyhold_amd.facade import FlexiCubes  # noqa: E402

gpu = pytest.mark.gpu
KEYS = ("v", "ldev", "s", "x", "alpha", "beta", "gamma")
# the referee's own float32 evaluation against its float64 one (measured, see above)
TOL_F32 = {"v": 3.86e-7, "ldev": 9.54e-8, "s": 3.79e-5, "x": 2.66e-4, "alpha": 9.12e-3, "beta": 8.18e-3, "gamma": 6.65e-3}


def _four_times_rounded_up(v):
    lead = 10.0 ** np.floor(np.log10(4 * v))
    return float(np.ceil(4 * v / lead - 1e-9) * lead)


TOL = {k: _four_times_rounded_up(v) for k, v in TOL_F32.items()}      # kernels against the referee
FIELDS = G.FUZZ + ("allcases", "tiny")
CASES = tuple((n, "rand") for n in FIELDS) + (("allcases", "ends"), ("fuzz1", "ends"))
EXTENT = 2.2                       # every field's grid spans 2.2 units


@functools.lru_cache(maxsize=None)
def topo(name):
    c = G.case(name)
    return W.Topology(c.s, c.res)


@functools.lru_cache(maxsize=None)
def weights(name, wset):
    c = G.case(name)
    return W.weights(c.res, 3000 + FIELDS.index(name), ends=(wset == "ends"))


@functools.lru_cache(maxsize=None)
def live(name, wset):
    """(V,) bool: the dual vertices whose crossings do not all coincide (float64 referee)."""
    c = G.case(name)
    return W.run(c.x, c.s, c.res, *weights(name, wset), topo=topo(name)).dmax >= 1e-6 * EXTENT / c.res


class Ref:
    """A case in one mode: the cotangents and the float64 referee, computed once, shared, never changed."""

    def __init__(self, name, wset, training):
        self.c, self.T, self.w, self.training = G.case(name), topo(name), weights(name, wset), training
        self.n_all = self.T.nv + (self.T.nq if training else 0)
        self.gv, self.gl = W.cotangents(self.n_all, self.T.nv, live(name, wset))
        self.r = self.run(torch.float64)

    def run(self, dtype, **kw):
        c = self.c
        return W.run(c.x, c.s, c.res, *self.w, training=self.training, dtype=dtype, g_verts=self.gv, g_ldev=self.gl, topo=self.T, **kw)


@functools.lru_cache(maxsize=None)
def ref(name, wset="rand", training=False):
    return Ref(name, wset, training)


def _measure(got, want, scale):
    if float(scale.max()) == 0.0:                 # no term lands anywhere (dL/dalpha on `tiny`): exact zeros or nothing
        return 0.0 if not bool(torch.as_tensor(got).any()) else float("inf")
    return G.measure(got.reshape(scale.shape), want, scale)[0]


def errs(r, verts, ldev, grads):
    """Errors of (verts, ldev, {input: gradient or None}) against the Result r, by key."""
    e = {"v": _measure(verts, r.verts.double(), r.scale_v), "ldev": _measure(ldev, r.ldev.double(), r.scale_l)}
    for k, g in grads.items():
        if r.grads[k] is not None and g is not None:
            e[k] = _measure(g, *r.grads[k])
    return e


def _fmt(e):
    return "  ".join(f"{k} {v:.3e}" for k, v in e.items())


# ---------------------------------------------------------------- CPU
def test_tolerances_follow_from_the_yardstick():
    want = {"v": 2e-6, "ldev": 4e-7, "s": 2e-4, "x": 2e-3, "alpha": 4e-2, "beta": 4e-2, "gamma": 3e-2}
    assert all(TOL[k] == pytest.approx(want[k], rel=1e-9) for k in KEYS), TOL
    for k in KEYS:
        assert 4 * TOL_F32[k] <= TOL[k] * (1 + 1e-12) < 10 * 4 * TOL_F32[k]


@pytest.mark.parametrize("name", FIELDS)
def test_unit_weights_are_the_oracle(name):
    """The referee with every weight absent, and with explicit ones, in float32: torch.equal to oracle.flexi_ref.flexicubes."""
    c = G.case(name)
    V, F, D = FR.flexicubes(c.x, c.s, c.res)
    C = c.res ** 3
    for w in ((None, None, None), (torch.ones(C, 8), torch.ones(C, 12), torch.ones(C))):
        r = W.run(c.x, c.s, c.res, *w, dtype=torch.float32, topo=topo(name))
        assert torch.equal(r.verts, V) and torch.equal(r.faces, F) and torch.equal(r.ldev, D)
        assert r.verts.dtype == torch.float32 and len(V) == topo(name).nv


def test_inputs_reach_what_they_were_built_for():
    """Conditions on the inputs (if one breaks, change the seed, never the condition)."""
    seen = {"second": set(), "first": set(), "tie": 0}
    for name, wset in CASES:
        r = ref(name, wset).r
        second, tie = r.g13 > r.g02, r.g13 == r.g02
        seen["second"] |= set(r.flip[second].tolist())
        seen["first"] |= set(r.flip[~second & ~tie].tolist())
        seen["tie"] += int(tie.sum())
        near = ((r.g13 - r.g02).abs() < 1e-6) & ~tie
        assert not bool(near.any()), name                       # no near-ties: float32 and float64 split alike
        al, be, ga = weights(name, wset)
        f32 = lambda v: float(np.float32(v))                    # the ends of the ranges as float32 has them
        assert f32(0.01) <= float(al.min()) and float(al.max()) <= f32(1.99) and f32(0.01) <= float(be.min()) and float(be.max()) <= f32(1.99)
        assert f32(0.005) <= float(ga.min()) and float(ga.max()) <= f32(0.995)
    r = ref("allcases").r
    second, tie = r.g13 > r.g02, r.g13 == r.g02
    print(f"allcases: {int(second.sum())} quads split along the second diagonal, {int((~second & ~tie).sum())} along the first, "
          f"{int(tie.sum())} exact ties, {int(r.flip.sum())} of {r.nq} reversed")
    # both splits, with both orientations each, and exact ties, on one field
    assert set(r.flip[second].tolist()) == {True, False} == set(r.flip[~second & ~tie].tolist()) and int(tie.sum()) > 100
    assert seen["second"] == {True, False} == seen["first"]
    c, T = G.case("allcases"), topo("allcases")
    multi = T.cubes[T.npc > 1]
    be = weights("allcases", "rand")[1][multi]
    assert len(multi) > 1000 and float((be.max(1)[0] - be.min(1)[0]).min()) > 0.1      # multi-patch cubes carry non-uniform beta
    assert len(weights("allcases", "rand")[2].unique()) == 8
    for w, ends in zip(weights("allcases", "ends"), ((0.01, 1.99), (0.01, 1.99), (0.005, 0.995))):
        assert sorted(w.unique().tolist()) == pytest.approx(sorted(ends))
    dead = sum(int((~live(n, w)).sum()) for n, w in CASES if w == "rand")
    print(f"{dead} dual vertices with coincident crossings carry no l_dev cotangent")
    assert bool(live("allcases", "rand").all()) and bool(live("tiny", "rand").all()) and 0 < dead < 2000
    t = ref("tiny", "rand", True).r
    assert t.nv == 8 and all(bool(torch.isfinite(g[0]).all()) for g in t.grads.values()) and float(t.grads["s"][0].abs().max()) > 1e20
    assert np.float32(1e-30) * np.float32(1e-30) == 0


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("out", ["verts", "ldev"])
def test_referee_matches_central_differences(training, out):
    """Float64 autograd through the leaf copies against central differences on three entries of each input, fuzz2 (res 12; multi-patch
    cubes), h = 1e-7: rounding 2.2e-16 |L| / h < 1e-7, truncation h^2 f''' / 6 far below; entries with |s| >= 0.02 so that no sign
    changes.  Bound 1e-5 of max(scale, 1)."""
    name = "fuzz2"
    c, T, (al, be, ga) = G.case(name), topo(name), weights(name, "rand")
    n_all = T.nv + (T.nq if training else 0)
    gv, gl = W.cotangents(n_all, T.nv, live(name, "rand"), seed=33)
    cot = dict(g_verts=gv) if out == "verts" else dict(g_ldev=gl)
    r = W.run(c.x, c.s, c.res, al, be, ga, training=training, topo=T, **cot)
    inputs = {"x": c.x.double(), "s": c.s.double(), "alpha": al.double(), "beta": be.double(), "gamma": ga.double()}
    assert T.nv > 100 and int((T.npc > 1).sum()) > 0

    def loss(**changed):
        a = dict(inputs, **changed)      # float64 values; the signs come from the topology passed in
        f = W.run(a["x"], a["s"], c.res, a["alpha"], a["beta"], a["gamma"], training=training, topo=T)
        return float((f.verts * gv.double()).sum()) if out == "verts" else float((f.ldev * gl.double()).sum())

    h, worst = 1e-7, 0.0
    if training and out == "ldev":
        assert not bool(r.grads["gamma"][1].any())                 # l_dev does not depend on gamma
    for k in ("s", "x", "alpha", "beta") + (("gamma",) if training and out == "verts" else ()):
        g, sc = r.grads[k]
        g, sc, flat = g.reshape(-1), sc.reshape(-1), inputs[k].reshape(-1)
        ok = sc > 0
        if k == "s":
            ok &= c.s.double().abs() >= 0.02
        idx = torch.nonzero(ok).reshape(-1)
        idx = idx[torch.argsort(sc[idx], descending=True)]         # the entries with the most on them: the 1st, 6th and 11th
        assert len(idx) >= 11, k
        for i in idx[:11:5].tolist():
            p, m = flat.clone(), flat.clone()
            p[i] += h
            m[i] -= h
            cd = (loss(**{k: p.reshape(inputs[k].shape)}) - loss(**{k: m.reshape(inputs[k].shape)})) / (2 * h)
            e = abs(cd - float(g[i])) / max(float(sc[i]), 1.0)
            worst = max(worst, e)
            assert e <= 1e-5, (k, i, cd, float(g[i]))
    if not training:
        assert r.grads["gamma"] is None
    print(f"fuzz2, training={training}, d{out}: central differences, worst {worst:.2e}")


def test_float32_yardstick():
    """The referee in float32 against itself in float64, every case, both modes: its worst values are TOL_F32 (a case that exceeds one
    means the header's figures are stale, not that the bound may grow unseen)."""
    worst = {k: (0.0, "") for k in KEYS}
    for name, wset in CASES:
        for training in (False, True):
            R = ref(name, wset, training)
            r32 = R.run(torch.float32)
            assert torch.equal(r32.faces, R.r.faces)
            assert all(bool(torch.isfinite(g[0]).all()) for g in r32.grads.values() if g is not None)
            e = errs(R.r, r32.verts, r32.ldev, {k: (None if g is None else g[0]) for k, g in r32.grads.items()})
            print(f"{name}/{wset}/{'training' if training else 'inference'}: {_fmt(e)}")
            for k, v in e.items():
                if v > worst[k][0]:
                    worst[k] = (v, f"{name}/{wset}/{int(training)}")
    print("worst: " + "  ".join(f"{k} {v:.3e} ({w}; TOL_F32 {TOL_F32[k]:.2e}, TOL {TOL[k]:.0e})" for k, (v, w) in worst.items()))
    for k in KEYS:
        assert 0.9 * TOL_F32[k] <= worst[k][0] <= TOL_F32[k], (k, worst[k])


def test_corrupted_referees_are_caught():
    """Teeth: each wrong operator is more than 100 x TOL from the referee on allcases -- l_dev taken to the weighted crossings (in l_dev),
    the gamma products taken before the quad is reversed (in the centres, and in the split), beta left out of B (in the vertices)."""
    R, Rt = ref("allcases"), ref("allcases", "rand", True)
    c, T, w = R.c, R.T, R.w
    bad = W.run(c.x, c.s, c.res, *w, topo=T, corrupt="ldev_weighted")
    e = _measure(bad.ldev, R.r.ldev, R.r.scale_l)
    print(f"ldev_weighted: l_dev {e:.3e}")
    assert e > 100 * TOL["ldev"] and torch.equal(bad.verts, R.r.verts)
    bad = W.run(c.x, c.s, c.res, *w, topo=T, corrupt="beta_not_in_B")
    e = _measure(bad.verts, R.r.verts, R.r.scale_v)
    print(f"beta_not_in_B: vertices {e:.3e}")
    assert e > 100 * TOL["v"]
    bad = W.run(c.x, c.s, c.res, *w, training=True, topo=T, corrupt="gamma_before_flip")
    e = _measure(bad.verts, Rt.r.verts, Rt.r.scale_v)
    print(f"gamma_before_flip: centres {e:.3e}")
    assert e > 100 * TOL["v"] and torch.equal(bad.verts[:T.nv], Rt.r.verts[:T.nv])
    assert not torch.equal(W.run(c.x, c.s, c.res, *w, topo=T, corrupt="gamma_before_flip").faces, R.r.faces)


# ---- the C ABI of libfoho_wflexi.so, on test_cabi.py's pattern
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "followmyhold_amd", "csrc", "foho_wflexi.h")


def test_signature_table_is_the_header():
    from test_cabi import prototypes
    scalars = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
               "float": ctypes.c_float, "char*": ctypes.c_char_p}
    protos = prototypes(HEADER)
    assert len(protos) == 6 == len({p[0] for p in protos}), [p[0] for p in protos]
    typed_by_loader = ("foho_wflexi_version", "foho_wflexi_last_error")
    assert set(WF._SIGNATURES) == {p[0] for p in protos} - set(typed_by_loader)
    for fn, ret, params in protos:
        if fn in typed_by_loader:
            continue
        restype, argtypes = WF._SIGNATURES[fn]
        assert restype is scalars[ret], (fn, ret, restype)
        assert len(argtypes) == len(params), (fn, params, argtypes)
        for i, (cdecl, t) in enumerate(zip(params, argtypes)):
            assert t is (ctypes.c_void_p if cdecl.endswith("*") else scalars[cdecl]), (fn, i, cdecl, t)
    assert _lib.SIDE_VERSIONS["wflexi"] == WF.VERSION == 100


def test_nothing_but_the_header_is_exported():
    from test_cabi import declared_functions
    _lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", WF.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3 and l.split()[-2] in ("T", "t", "W", "V", "B", "D"))
    exported = [n for n in exported if not n.startswith(("_init", "_fini", "__bss_start", "_edata", "_end", "__hip_"))]
    assert exported == declared_functions(HEADER), sorted(set(exported) ^ set(declared_functions(HEADER)))


def test_entry_points_validate_arguments_without_a_gpu():
    _lib.build()
    L = WF.lib()
    assert L.foho_wflexi_version() == 100
    assert L.foho_wflexi_workspace_bytes(0, 10) == 0 == L.foho_wflexi_workspace_bytes(257, 10) == L.foho_wflexi_workspace_bytes(8, -1)
    assert L.foho_wflexi_workspace_bytes(256, 1 << 20) > 6 * 256 ** 3 and L.foho_wflexi_bwd_bytes(1000) >= 384000 and L.foho_wflexi_bwd_bytes(-1) == 0
    one, big = ctypes.c_void_p(256), ctypes.c_size_t(1 << 40)      # a non-null pointer that is never dereferenced: every call is refused before a launch

    def refused(status, *words):
        msg = L.foho_wflexi_last_error().decode()
        assert status < 0 and all(w in msg for w in words), (status, msg)

    def fwd(x=one, res=8, vc=10, fc=10, ws=one, wb=big):
        return L.foho_wflexi_fwd(x, one, None, None, None, res, 0, one, vc, one, fc, None, one, ws, wb, None)

    refused(fwd(x=None), "foho_wflexi_fwd", "null")
    refused(fwd(res=257), "resolution")
    refused(fwd(res=0), "resolution")
    refused(fwd(vc=-1), "capacity")
    refused(fwd(wb=L.foho_wflexi_workspace_bytes(8, 10) - 1), "workspace too small")

    def bwd(res=8, nv=40, na=40, nc=10, ga=None, al=None, gs=one, sc=one, sb=big, wb=big, vc=64, training=0, verts=one):
        return L.foho_wflexi_bwd(one, one, al, None, None, res, training, verts, nv, na, nc, one, None, gs, None, ga, None, None, one, wb, vc, sc,
                                 sb, None)

    refused(bwd(res=300), "foho_wflexi_bwd", "resolution")
    refused(bwd(nc=41), "counts")
    refused(bwd(na=39), "counts")
    refused(bwd(vc=39), "counts")
    refused(bwd(ga=one), "weight that is NULL")
    refused(bwd(training=1, verts=None), "vertices")
    refused(bwd(sb=L.foho_wflexi_bwd_bytes(10) - 1), "scratch too small")
    refused(bwd(wb=L.foho_wflexi_workspace_bytes(8, 64) - 1), "workspace too small")
    assert bwd(nc=0, nv=0, na=0) == 0                             # nothing to do is success without a launch


# ---------------------------------------------------------------- GPU
def _op(R, need=("x", "s", "alpha", "beta", "gamma"), **kw):
    """ops.flexicubes_weighted on the case with the listed inputs requiring grad, backward with the case's cotangents
    -> (verts, faces, l_dev, {input: leaf})."""
    from followmyhold_amd import ops
    c = R.c
    t = dict(zip(("x", "s", "alpha", "beta", "gamma"), (c.x, c.s) + tuple(R.w)))
    t = {k: v.cuda().requires_grad_(k in need) for k, v in t.items()}
    v, f, l = ops.flexicubes_weighted(t["x"], t["s"], c.res, t["alpha"], t["beta"], t["gamma"], training=R.training, **kw)
    ((v * R.gv.cuda()).sum() + (l * R.gl.cuda()).sum()).backward()
    return v, f, l, t


def _closed(faces):
    e = torch.sort(torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)[0]
    return bool((torch.unique(e, dim=0, return_counts=True)[1] == 2).all())


@gpu
@pytest.mark.parametrize("name", FIELDS)
def test_hip_unit_weights_are_flexicubes_bitwise(name):
    from followmyhold_amd import ops
    c = G.case(name)
    x, s, C = c.x.cuda(), c.s.cuda(), c.res ** 3
    v0, f0, l0 = ops.flexicubes(x, s, c.res)
    ones = (torch.ones(C, 8, device="cuda"), torch.ones(C, 12, device="cuda"), torch.ones(C, device="cuda"))
    for w in ((None, None, None), ones):
        v, f, l = ops.flexicubes_weighted(x, s, c.res, *w)
        assert len(v) == topo(name).nv and f.dtype == torch.int64
        assert torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(l, l0)


@gpu
@pytest.mark.parametrize("training", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("name,wset", [c for c in CASES if c[0] != "tiny"])
def test_hip_forward_and_gradients_match_the_referee(name, wset, training):
    """Faces exactly the referee's; vertices, centres, l_dev and the gradients to all five inputs within TOL; exact zeros where no term
    lands; no gradient to gamma outside training mode; with s alone requiring grad the others' .grad stay None."""
    R = ref(name, wset, training)
    r, T = R.r, R.T
    v, f, l, t = _op(R)
    assert torch.equal(f.cpu(), r.faces) and not f.requires_grad and l.requires_grad
    assert v.shape == (R.n_all, 3) and l.shape == (T.nv,)
    if training:
        assert len(v) == T.nv + T.nq and len(f) == 4 * T.nq
    else:
        assert len(f) == 2 * T.nq and t["gamma"].grad is None
    grads = {k: (None if t[k].grad is None else t[k].grad.cpu()) for k in t}
    e = errs(r, v.detach().cpu(), l.detach().cpu(), grads)
    print(f"{name}/{wset}/{'training' if training else 'inference'} ({T.nv} vertices, {T.nq} quads): {_fmt(e)}")
    assert set(e) == set(KEYS) - (set() if training else {"gamma"})
    for k, val in e.items():
        assert val <= TOL[k], (k, val, TOL[k])
    for k, g in grads.items():
        if g is not None:
            rows = g.reshape(len(r.lands[k]), -1)                # (entries, 1), or (grid points, 3) for x
            assert bool(torch.isfinite(g).all()) and not bool(rows[~r.lands[k]].any()), k
            assert not bool(r.grads[k][1].reshape(len(r.lands[k]), -1)[~r.lands[k]].any())
    v1, _, _, t1 = _op(R, need=("s",))
    assert torch.equal(v1, v) and all(t1[k].grad is None for k in ("x", "alpha", "beta", "gamma"))
    assert _measure(t1["s"].grad.cpu(), *r.grads["s"]) <= TOL["s"]


@gpu
def test_hip_training_mesh_of_a_closed_field_is_closed():
    """A sphere inside the grid, res 12: V + Q vertices, 4 Q faces, every edge shared by two faces, in both modes."""
    from followmyhold_amd import ops
    res = 12
    x = FR.construct_voxel_grid(res)[0] * 2.2
    s = x.norm(dim=1) - 0.8
    T = W.Topology(s, res)
    al, be, ga = W.weights(res, 77)
    for training in (False, True):
        v, f, l = ops.flexicubes_weighted(x.cuda(), s.cuda(), res, al.cuda(), be.cuda(), ga.cuda(), training=training)
        assert len(v) == T.nv + (T.nq if training else 0) and len(f) == (4 if training else 2) * T.nq and len(l) == T.nv
        assert _closed(f.cpu()) and int(f.max()) == len(v) - 1 and int(f.min()) == 0


@gpu
@pytest.mark.parametrize("training", [False, True], ids=["inference", "training"])
def test_hip_tiny_is_finite_where_d_squared_underflows(training):
    R = ref("tiny", "rand", training)
    v, f, l, t = _op(R)
    grads = {k: (None if t[k].grad is None else t[k].grad.cpu()) for k in t}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None) and float(grads["s"].abs().max()) > 1e20
    e = errs(R.r, v.detach().cpu(), l.detach().cpu(), grads)
    print(f"tiny/{'training' if training else 'inference'}: {_fmt(e)}")
    assert torch.equal(f.cpu(), R.r.faces)
    for k, val in e.items():
        assert val <= TOL[k], (k, val)


@gpu
def test_hip_gradients_are_bitwise_repeatable():
    """Two backward runs, the second on another stream: all five gradients bitwise equal."""
    R = ref("allcases", "rand", True)
    first = {k: t.grad.clone() for k, t in _op(R)[3].items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again = {k: t.grad for k, t in _op(R)[3].items()}
    side.synchronize()
    for k in first:
        assert int(torch.count_nonzero(first[k])) > 1000 and torch.equal(first[k], again[k]), k


@gpu
@pytest.mark.parametrize("training", [False, True], ids=["inference", "training"])
def test_hip_capacity_overflow_ends_with_the_same_outputs(training):
    R = ref("fuzz3", "rand", training)
    v, f, l, t = _op(R)
    v1, f1, l1, t1 = _op(R, verts_cap=1, faces_cap=1)
    assert torch.equal(v, v1) and torch.equal(f, f1) and torch.equal(l, l1) and len(v) > 100
    assert all(torch.equal(t[k].grad, t1[k].grad) for k in t if t[k].grad is not None)


@gpu
def test_hip_facade_with_zero_raw_weights_is_flexicubes_bitwise():
    """tanh(0) 0.99 + 1 = 1, sigmoid(0) 0.99 + 0.005 equal everywhere: the default mesh.  (NotImplementedError before this operator.)"""
    from followmyhold_amd import ops
    c = G.case("fuzz5")
    C = c.res ** 3
    x, s = c.x.cuda(), c.s.cuda()
    fc = FlexiCubes("cuda")
    cube = fc.construct_voxel_grid(c.res)[1]
    raw = (torch.zeros(C, 12, device="cuda"), torch.zeros(C, 8, device="cuda"), torch.zeros(C, device="cuda"))
    v, f, l = fc(x, s, cube, c.res, beta_fx12=raw[0], alpha_fx8=raw[1], gamma_f=raw[2], training=False)
    v0, f0, l0 = ops.flexicubes(x, s, c.res)
    assert len(v) > 100 and torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(l, l0)
    v0, f0, l0 = fc(x, s, cube, c.res)                              # the call without weights is ops.flexicubes as before
    assert torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(l, l0)


def _normalise(raw_beta, raw_alpha, raw_gamma):
    """The façade's normalisation, restated: (alpha, beta in THIS repository's edge order, gamma)."""
    k2o = FlexiCubes.KAOLIN_EDGE_TO_OURS
    beta = torch.empty_like(raw_beta)
    beta[:, list(k2o)] = torch.tanh(raw_beta) * 0.99 + 1            # kaolin's column k is our edge k2o[k]
    return torch.tanh(raw_alpha) * 0.99 + 1, beta, torch.sigmoid(raw_gamma) * 0.99 + 0.005


def test_kaolin_edge_permutation_is_a_permutation_of_the_edge_table():
    """kaolin's cube_edges, as recalled, against this repository's edge table: column k joins the same two corners as our edge k2o[k]."""
    kaolin = [(0, 1), (1, 5), (4, 5), (0, 4), (2, 3), (3, 7), (6, 7), (2, 6), (2, 0), (3, 1), (7, 5), (6, 4)]
    k2o = FlexiCubes.KAOLIN_EDGE_TO_OURS
    assert sorted(k2o) == list(range(12))
    assert [tuple(sorted(e)) for e in kaolin] == [FR.EDGES[o] for o in k2o]


@gpu
def test_hip_facade_training_gradients_reach_the_raw_weights():
    """Raw random weights, training=True: gradients at the raw tensors agree with the referee's at the normalised weights chained, in
    float64, through the normalisation and the column permutation."""
    name = "fuzz4"
    c, T = G.case(name), topo(name)
    C = c.res ** 3
    g = torch.Generator().manual_seed(91)
    raw = [torch.randn(C, 12, generator=g), torch.randn(C, 8, generator=g), torch.randn(C, generator=g)]
    dev = [t.cuda().requires_grad_(True) for t in raw]
    fc = FlexiCubes("cuda")
    with torch.no_grad():
        al, be, ga = (t.cpu() for t in _normalise(*[t.detach() for t in dev]))                 # the float32 weights the operator gets
    lv = W.run(c.x, c.s, c.res, al, be, ga, topo=T).dmax >= 1e-6 * EXTENT / c.res
    gv, gl = W.cotangents(T.nv + T.nq, T.nv, lv, seed=92)
    r = W.run(c.x, c.s, c.res, al, be, ga, training=True, topo=T, g_verts=gv, g_ldev=gl)
    v, f, l = fc(c.x.cuda(), c.s.cuda(), None, c.res, beta_fx12=dev[0], alpha_fx8=dev[1], gamma_f=dev[2], training=True)
    ((v * gv.cuda()).sum() + (l * gl.cuda()).sum()).backward()
    assert torch.equal(f.cpu(), r.faces)
    r64 = [t.double().requires_grad_(True) for t in raw]
    n64 = _normalise(*r64)
    for k, out, leaf, got in (("alpha", n64[0], r64[1], dev[1]), ("beta", n64[1], r64[0], dev[0]), ("gamma", n64[2], r64[2], dev[2])):
        gr, sc = (t.reshape(out.shape) for t in r.grads[k])
        want = torch.autograd.grad(out, leaf, gr, retain_graph=True)[0]
        scale = torch.autograd.grad(out, leaf, sc, retain_graph=True)[0].abs()
        e = _measure(got.grad.cpu(), want, scale)
        print(f"facade training, raw {k}: {e:.3e} (TOL {TOL[k]:.0e})")
        assert float(want.abs().max()) > 0 and e <= TOL[k], (k, e)


@gpu
def test_hip_end_to_end_optimisation_of_the_weights():
    """res-8 sphere, s fixed, twenty Adam steps on raw alpha and beta alone through the façade: the loss mean((|v| - r)^2) +
    l_dev.mean() ends below where it started, and the referee at the final weights reproduces the operator's vertices within TOL."""
    res, rad = 8, 0.8
    fc = FlexiCubes("cuda")
    x = FR.construct_voxel_grid(res)[0] * 2.2
    s = x.norm(dim=1) - rad
    xg, sg = x.cuda(), s.cuda()
    raw_b = torch.zeros(res ** 3, 12, device="cuda", requires_grad=True)
    raw_a = torch.zeros(res ** 3, 8, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([raw_a, raw_b], lr=0.05)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        v, f, l = fc(xg, sg, None, res, beta_fx12=raw_b, alpha_fx8=raw_a)
        loss = ((v.norm(dim=1) - rad) ** 2).mean() + l.mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"end to end: loss {losses[0]:.5e} -> {losses[-1]:.5e}")
    assert losses[-1] < losses[0] and float(raw_a.detach().abs().max()) > 0 and float(raw_b.detach().abs().max()) > 0
    with torch.no_grad():
        v, f, l = fc(xg, sg, None, res, beta_fx12=raw_b, alpha_fx8=raw_a)
        al, be, _ = (t.cpu() for t in _normalise(raw_b, raw_a, torch.zeros(res ** 3, device="cuda")))
    r = W.run(x, s, res, al, be, None)
    e = errs(r, v.cpu(), l.cpu(), {})
    print(f"end to end, final weights against the referee: {_fmt(e)}")
    assert torch.equal(f.cpu(), r.faces) and e["v"] <= TOL["v"] and e["ldev"] <= TOL["ldev"]


@gpu
def test_hip_error_paths():
    from followmyhold_amd import ops
    c = G.case("fuzz0")
    x, s, C = c.x.cuda(), c.s.cuda(), c.res ** 3
    with pytest.raises(_lib.FohoError, match="beta"):
        ops.flexicubes_weighted(x, s, c.res, beta=torch.ones(C, 11, device="cuda"))
    with pytest.raises(_lib.FohoError, match="CUDA"):
        ops.flexicubes_weighted(x, c.s, c.res)
    with pytest.raises(_lib.FohoError, match="resolution"):
        ops.flexicubes_weighted(x, s, 257)
    with pytest.raises(_lib.FohoError, match="alpha"):
        ops.flexicubes_weighted(x, s, c.res, alpha=torch.ones(C, device="cuda"))
