"""MANO-shaped linear blend skinning (foho_lbs_fwd / foho_lbs_bwd: ops.lbs, ops.LbsModel) against a float64 closed-form referee:
forward and every gradient, sparse skinning weights, every tile path of the pose-blend GEMM.

tests/lbs_ref64.py evaluates the smplx formulas and their reverse sweep down the kinematic tree in numpy.  Errors are measured per
batch element b against the float64 referee, and the worst over the batch is reported:
  verts, joints   max |d| / max |ref_b|
  g_betas         max |d| / max |ref g_betas_b|
  g_rot           per joint block (b, j):  max |d| / max(max |ref block|, 1e-3 max |ref g_rot_b|)
(the root's block of g_rot is ~1.5, a fingertip's 0.02 .. 0.06: one norm over the tensor, the measure of test_ops_gpu.py, does not see a
fingertip block that is 0.5 % wrong -- test_the_old_measure_is_blind_to_a_fingertip_block).  The floor serves blocks that are zero.

Cases (V, keep, B, pose scale in rad; `keep` = skinning weights kept per vertex, the rest exact zeros, lbs_ref64.model):
  a   778  dense / 3    3   0.3   use_mfma 0 and 1: VALU path; one 16-row tile with 13 padded rows; the wave skip of k_lbs_bwd_verts
  b   778  3           17   0.3   automatic: second 16-row tile with one live row (clamped row address)
  c     5  2            3   0.3   3V = 15 < 16: a single partial tile, the N - 1 clamps
  d    22  3    128 / 130   0.3   k_lbs_poseblend_mfma64<1> at its threshold; third row tile with 2 rows; 3V = 66 = 64 + 2
  e    86  3  4096 / 4097   0.3   k_lbs_poseblend_mfma64<4>: 3V = 258, the second column workgroup has 2 live columns in strip 0 and
                                  breaks; ragged last row tile
  f   778  3            2   1.5   large rotations, VALU path

Tolerances.  TOL_F32 is the worst error of the referee's own float32 evaluation against its float64 one over the cases' inputs:
  measured  verts 6.33e-7 (f; the others 1.2e-7 .. 4.2e-7)      joints 7.36e-7 (f; 1.6e-7 .. 6.9e-7)
            g_betas 2.31e-6 (b; 2.4e-7 .. 2.3e-6)               g_rot 8.15e-6 (a dense; 1.2e-6 .. 5.5e-6)
TOL, the kernel's bound, is 4 x TOL_F32 rounded up to one significant digit -- verts 3e-6, joints 3e-6, g_betas 1e-5, g_rot 4e-5: the
kernel sums in another order than the referee (per thread, per wave, LDS and global float atomics in no fixed order).  Neither number
comes from what the kernel achieves; a kernel that needs more is a finding.  The float64 referee against float64 torch autograd of
oracle.lbs_ref.lbs is within 1.8e-14 (bound 1e-12).

CPU: referee == float64 autograd, central differences, three corrupted referees that must be caught, the conditions on the inputs,
the float32 yardstick, four known answers that involve no restatement, the power of the measure, LbsModel's refusal of a parents
array the kernels cannot walk.  GPU: the cases above; on case a the cotangent on one output only (through autograd and with the
library's null grad_joints), two backward calls from one forward, float64 / non-contiguous inputs; the three matrix-core kernels
bit for bit against one another at V = 22 and 86; the known answers."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lbs_ref64 as G  # noqa: E402
from oracle import lbs_ref  # noqa: E402

gpu = pytest.mark.gpu
QUANT = ("verts", "joints", "g_betas", "g_rot")
TOL_F32 = {"verts": 6.4e-7, "joints": 7.4e-7, "g_betas": 2.4e-6, "g_rot": 8.2e-6}   # referee float32 against float64 (measured, see above)
TOL = {"verts": 3e-6, "joints": 3e-6, "g_betas": 1e-5, "g_rot": 4e-5}               # kernel against referee: 4 x TOL_F32, one digit, up
TOL_AUTOGRAD = 1e-12
TOL_EXACT = 1e-13                                                                   # float64 referee against a closed-form answer
SEED = 1
#        name       V  keep    B  scale
CASES = {"a_dense": (778, None, 3, 0.3), "a_keep3": (778, 3, 3, 0.3), "b": (778, 3, 17, 0.3), "c": (5, 2, 3, 0.3),
         "d128": (22, 3, 128, 0.3), "d130": (22, 3, 130, 0.3), "e4096": (86, 3, 4096, 0.3), "e4097": (86, 3, 4097, 0.3),
         "f": (778, 3, 2, 1.5)}
GPU_RUNS = [("a_dense", 0), ("a_dense", 1), ("a_keep3", 0), ("a_keep3", 1), ("b", -1), ("c", 1), ("d128", 1), ("d130", 1),
            ("e4096", 1), ("e4097", 1), ("f", 0)]
SPARSE = sorted({(V, keep) for V, keep, _, _ in CASES.values() if keep is not None})
_BMAX = {}
for _V, _keep, _B, _scale in CASES.values():
    _BMAX[(_V, _keep, _scale)] = max(_B, _BMAX.get((_V, _keep, _scale), 0))


@functools.lru_cache(maxsize=None)
def _ref_full(V, keep, scale):
    """The float64 referee on the longest batch of (V, keep, scale); batch elements are independent, shorter cases are prefixes."""
    b, r, gv, gj = G.inputs(V, _BMAX[(V, keep, scale)], SEED, scale)
    out = G.lbs(b, r, G.model(V, SEED, keep), gv, gj)
    for a in out:
        a.setflags(write=False)
    return out


def case(name):
    """-> model, (betas, rot, g_verts, g_joints), referee (verts, joints, g_betas, g_rot)."""
    V, keep, B, scale = CASES[name]
    return G.model(V, SEED, keep), G.inputs(V, B, SEED, scale), tuple(a[:B] for a in _ref_full(V, keep, scale))


def _report(what, e, tol=TOL):
    print(f"{what}: " + "  ".join(f"{k} {v:.2e} ({v / tol[k]:.2f} of the bound)" for k, v in e.items()))


def _within(e, tol=TOL):
    return all(v <= tol[k] for k, v in e.items())


def _lbs_model(m, **kw):
    """ops.LbsModel of writable copies (the cached models are read-only, and torch warns when it wraps such an array)."""
    from followmyhold_amd import ops
    return ops.LbsModel({k: np.array(v) for k, v in m.items()}, **kw)


def _autograd64(betas, rot, m, gv, gj):
    mt = {k: torch.tensor(np.asarray(v)) for k, v in m.items()}
    bt, rt = torch.tensor(betas).double().requires_grad_(True), torch.tensor(rot).double().requires_grad_(True)
    v, j = lbs_ref.lbs(bt, rt, mt)
    ((v * torch.tensor(gv).double()).sum() + (j * torch.tensor(gj).double()).sum()).backward()
    return v.detach().numpy(), j.detach().numpy(), bt.grad.numpy(), rt.grad.numpy()


# ---------------------------------------------------------------- CPU
def test_tolerances_follow_from_the_yardstick():
    for k in QUANT:
        lead = 10.0 ** np.floor(np.log10(4 * TOL_F32[k]))
        assert TOL[k] == pytest.approx(np.ceil(4 * TOL_F32[k] / lead - 1e-9) * lead, rel=1e-12)


@pytest.mark.parametrize("V,keep", SPARSE)
def test_sparse_models_reach_the_wave_skip(V, keep):
    """Conditions on the models (if one breaks, change the seed, never the condition): with the kernel's wave layout every sparse
    model has a wave-joint pair that k_lbs_bwd_verts skips, one with zero and non-zero lanes, and one with every lane live.  Every
    joint owns a vertex where the model has more than one wave; in a single wave a skipped pair IS a joint without a vertex, so there
    the two sets must coincide (a joint's block of g_rot then comes from the joint cotangent, its subtree and the pose feature)."""
    w = G.model(V, SEED, keep)["lbs_weights"]
    assert ((w != 0).sum(1) == keep).all() and w.dtype == np.float32
    assert np.abs(w.astype(np.float64).sum(1) - 1).max() < 2e-7
    skipped, mixed, full = G.wave_joint_pairs(w)
    owned = (w != 0).sum(0)
    print(f"V {V} keep {keep}: {skipped} skipped, {mixed} mixed, {full} full wave-joint pairs; vertices per joint {owned.tolist()}")
    assert skipped >= 1 and mixed >= 1 and full >= 1
    if V > 64:
        assert (owned >= 1).all()
    else:
        assert int((owned == 0).sum()) == skipped and (owned >= 1).sum() >= 5
    if V == 778:        # 13 waves x 16 joints; pinned so that a change of synthetic.mano_like_model shows here
        assert (skipped, mixed, full) == (61, 146, 1) and owned.min() >= 20
        assert (G.model(778, SEED)["lbs_weights"] != 0).all()       # the dense model never skips


@pytest.mark.parametrize("name", CASES)
def test_every_block_of_g_rot_is_above_the_floor(name):
    """With cotangents on both outputs no joint block is exempt: the floor of the measure must not be what a block is measured by."""
    _, _, ref = case(name)
    block, floor = G.rot_block_scale(ref[3])
    print(f"{name}: smallest block / floor {float((block / floor).min()):.1f}")
    assert (block > floor).all()


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][2] <= 130])
def test_referee_equals_float64_autograd_of_the_oracle(name):
    """Two derivations: the closed-form sweep and torch autograd through oracle.lbs_ref.lbs, both in float64."""
    m, (b, r, gv, gj), ref = case(name)
    e = G.measure(ref, _autograd64(b, r, m, gv, gj))
    _report(f"{name}: referee against float64 autograd", e, dict.fromkeys(QUANT, TOL_AUTOGRAD))
    assert max(e.values()) <= TOL_AUTOGRAD, e


def test_referee_matches_central_differences():
    """L = <verts, g_v> + <joints, g_j> through the oracle's forward in float64.  L is a polynomial of degree 2 in every entry of betas
    and of rot (a rotation enters once through the pose feature and once through the chain), so the central difference has no
    truncation error; rounding is 2.2e-16 |L| / h ~ 1e-11 at h = 1e-3, |L| ~ 50, against blocks of 0.02 and more: bound 1e-8."""
    m, (b, r, gv, gj), ref = case("a_keep3")
    mt = {k: torch.tensor(np.asarray(v)) for k, v in m.items()}
    gvt, gjt, h = torch.tensor(gv).double(), torch.tensor(gj).double(), 1e-3

    def L(bb, rr):
        v, j = lbs_ref.lbs(torch.tensor(bb), torch.tensor(rr), mt)
        return float((v * gvt).sum() + (j * gjt).sum())

    b64, r64 = b.astype(np.float64), r.astype(np.float64)
    worst = 0.0
    for bi, l in ((0, 0), (1, 4), (2, 9)):
        bp, bm = b64.copy(), b64.copy()
        bp[bi, l] += h
        bm[bi, l] -= h
        fd = (L(bp, r64) - L(bm, r64)) / (2 * h)
        worst = max(worst, abs(fd - ref[2][bi, l]) / np.abs(ref[2][bi]).max())
    for bi, j, a, c in ((0, 0, 0, 1), (1, 0, 2, 2), (0, 5, 1, 0), (2, 5, 0, 0), (1, 15, 2, 1), (2, 15, 1, 1), (0, 9, 0, 2)):   # root, mid, tips
        rp, rm = r64.copy(), r64.copy()
        rp[bi, j, a, c] += h
        rm[bi, j, a, c] -= h
        fd = (L(b64, rp) - L(b64, rm)) / (2 * h)
        worst = max(worst, abs(fd - ref[3][bi, j, a, c]) / np.abs(ref[3][bi, j]).max())
    print(f"referee against central differences: worst {worst:.2e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("corrupt", G.CORRUPTIONS)
def test_corrupted_referees_are_caught(corrupt):
    """Teeth: each wrong formula leaves the kernel's bound by orders of magnitude, on the dense and on the sparse model."""
    for name in ("a_dense", "a_keep3", "d130"):
        m, (b, r, gv, gj), ref = case(name)
        e = G.measure(G.lbs(b, r, m, gv, gj, corrupt=corrupt), ref)
        _report(f"{name}: {corrupt}", e)
        assert e["verts"] == 0 and e["joints"] == 0
        assert e["g_rot"] > 1e3 * TOL["g_rot"]
        assert not _within(e)


def test_float32_yardstick():
    """The referee evaluated in float32 against itself in float64 on exactly the cases' inputs: what float32 arithmetic achieves on
    these formulas.  Its worst value is TOL_F32 (a case that exceeds it means the header's figures are stale, not that the bound
    may grow unseen)."""
    worst = dict.fromkeys(QUANT, 0.0)
    for name in CASES:
        m, (b, r, gv, gj), ref = case(name)
        r32 = G.lbs(b, r, m, gv, gj, dtype=np.float32)
        assert all(np.isfinite(a).all() for a in r32)
        e = G.measure(r32, ref)
        _report(f"{name}: float32 referee against float64", e, TOL_F32)
        worst = {k: max(worst[k], e[k]) for k in QUANT}
    _report("worst", worst, TOL_F32)
    for k in QUANT:
        assert 0.9 * TOL_F32[k] <= worst[k] <= TOL_F32[k], (k, worst[k])


def test_the_old_measure_is_blind_to_a_fingertip_block():
    """Power: a 0.5 % error in one fingertip block of g_rot passes the norm-relative 1e-4 of test_ops_gpu.py and fails here."""
    _, _, ref = case("a_dense")
    bad = ref[3].copy()
    bad[0, 15] *= 1.005
    old = float(np.linalg.norm(bad - ref[3]) / np.linalg.norm(ref[3]))
    new = G.measure_rot(bad, ref[3])
    print(f"0.5 % on block (0, 15): norm-relative {old:.2e} (old bound 1e-4), per-block measure {new:.2e} (bound {TOL['g_rot']:.0e})")
    assert old < 1e-4
    assert new == pytest.approx(5e-3, rel=1e-6) and new > 100 * TOL["g_rot"]


# ---- known answers: exact formulas in float64, no restatement of lbs() involved.  Each returns what to feed and what must come out.
def _known_answers():
    """-> list of (name, model, betas, rot, expected verts, expected joints).  The float32 weights of a vertex sum to s_v = 1 within
    6e-8, and verts_v = sum_j W_vj (...) carries that sum: the exact answer of a rigid motion M is s_v M(v) (s_v = 1 for one-hot rows)."""
    out = []
    f64 = lambda a: np.asarray(a, np.float64)
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (1, 16, 3, 3)).copy()
    # 1. zero betas, identity rotations: the template, Jreg . template (and a pose feature of exactly 0: the posedirs stay in)
    m = G.model(778, SEED, 3)
    s = f64(m["lbs_weights"]).sum(1)[:, None]
    T, Jreg = f64(m["v_template"]), f64(m["J_regressor"])
    out.append(("template", m, np.zeros((1, 10), np.float32), eye, (s * T)[None], (Jreg @ T)[None]))
    # 2. posedirs zeroed, the root alone rotated: R (x - J0) + J0 for every vertex and every joint
    betas = G.inputs(778, 1, SEED)[0]
    m2 = dict(m, posedirs=np.zeros_like(m["posedirs"]))
    vs = T + np.einsum("vcl,l->vc", f64(m["shapedirs"]), f64(betas[0]))
    J = Jreg @ vs
    R = G.rodrigues(np.array([0.7, -1.1, 0.4])).astype(np.float32)
    rot = eye.copy()
    rot[0, 0] = R
    rigid = lambda x, c: (x - c) @ f64(R).T + c
    out.append(("root", m2, betas, rot, (s * rigid(vs, J[0]))[None], rigid(J, J[0])[None]))
    # 3. posedirs zeroed, one-hot weights, one mid-finger joint rotated: its subtree moves rigidly about J_j, the rest stays
    j, sub = 5, (5, 6)
    assert G.PARENTS[5] == 4 and G.PARENTS[6] == 5 and 5 not in G.LEAVES and [i for i in range(16) if G.PARENTS[i] == 6] == []
    m3 = G.model(778, SEED, 1)
    own = np.argmax(m3["lbs_weights"], 1)
    assert set(np.unique(m3["lbs_weights"]).tolist()) == {0.0, 1.0} and all((own == i).sum() >= 10 for i in sub)
    m3 = dict(m3, posedirs=np.zeros_like(m3["posedirs"]))
    rot = eye.copy()
    rot[0, j] = R
    moved = np.isin(own, sub)[:, None]
    out.append(("mid_finger", m3, betas, rot, np.where(moved, rigid(vs, J[j]), vs)[None],
                np.where(np.isin(np.arange(16), sub)[:, None], rigid(J, J[j]), J)[None]))
    return out


def test_known_answers_referee():
    """1-3 of the known answers, and 4: the gradient of sum(joints) with respect to a leaf joint's rotation is exactly zero."""
    for name, m, betas, rot, v_exp, j_exp in _known_answers():
        v, j, _, _ = G.lbs(betas, rot, m)
        e = G.measure((v, j, None, None), (v_exp, j_exp, None, None))
        print(f"known answer {name}: verts {e['verts']:.1e} joints {e['joints']:.1e}")
        assert max(e.values()) <= TOL_EXACT, (name, e)
    m, (b, r, _, _), _ = case("a_keep3")
    _, _, gb, gr = G.lbs(b, r, m, None, np.ones((3, 16, 3), np.float32))
    assert (gr[:, list(G.LEAVES)] == 0).all() and all(np.abs(gr[:, i]).max() > 0 for i in range(16) if i not in G.LEAVES)
    assert np.abs(gb).max() > 0


def test_lbs_model_refuses_parents_the_kernels_cannot_walk():
    """k_lbs_joints walks the joints in index order: a parent at or after its child would be read before it is written.  The check
    precedes the upload, so it needs no device."""
    from followmyhold_amd import ops
    from followmyhold_amd._lib import FohoError
    m = G.model(5, SEED)
    good = list(G.PARENTS)
    for i, p in ((0, 0), (0, 3), (4, -1), (7, 7), (2, 9), (15, 16)):
        bad = good.copy()
        bad[i] = p
        with pytest.raises(FohoError, match="parents"):
            _lbs_model(dict(m, parents=np.array(bad)), device="cpu")
    with pytest.raises(FohoError, match="parents"):
        _lbs_model(dict(m, parents=np.array(good[:15])), device="cpu")
    assert _lbs_model(m, device="cpu").V == 5        # the MANO tree itself passes


# ---------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _device_model(V, keep):
    return _lbs_model(G.model(V, SEED, keep))


def _kernel(model, betas, rot, gv, gj, use_mfma):
    """ops.lbs forward and backward through autograd -> (verts, joints, g_betas, g_rot) as numpy; gv / gj None = output unused."""
    from followmyhold_amd import ops
    bd, rd = torch.tensor(betas).cuda().requires_grad_(True), torch.tensor(rot).cuda().requires_grad_(True)
    verts, joints = ops.lbs(bd, rd, model, use_mfma=use_mfma)
    loss = 0
    if gv is not None:
        loss = loss + (verts * torch.tensor(gv).cuda()).sum()
    if gj is not None:
        loss = loss + (joints * torch.tensor(gj).cuda()).sum()
    loss.backward()
    return tuple(t.detach().cpu().numpy() for t in (verts, joints, bd.grad, rd.grad))


@gpu
@pytest.mark.parametrize("name,use_mfma", GPU_RUNS)
def test_kernel_against_the_referee(name, use_mfma):
    V, keep, B, _ = CASES[name]
    _, (b, r, gv, gj), ref = case(name)
    got = _kernel(_device_model(V, keep), b, r, gv, gj, use_mfma)
    assert got[0].shape == (B, V, 3) and got[1].shape == (B, 16, 3) and got[2].shape == (B, 10) and got[3].shape == (B, 16, 3, 3)
    e = G.measure(got, ref)
    _report(f"{name} use_mfma {use_mfma}: kernel against referee", e)
    assert _within(e), e


@gpu
@pytest.mark.parametrize("V,keep,B4", [(22, 3, 4096), (86, 3, 4097)])
def test_matrix_core_kernels_agree_bitwise(V, keep, B4):
    """Same k-chunking in k_lbs_poseblend_mfma (B < 128), _mfma64<1> (B < 4096) and _mfma64<4>: one batch prefix, the same bits."""
    from followmyhold_amd import ops
    model = _device_model(V, keep)
    b, r, _, _ = G.inputs(V, B4, SEED, 0.3)
    bd, rd = torch.tensor(b).cuda(), torch.tensor(r).cuda()
    v4, j4 = ops.lbs(bd, rd, model, use_mfma=1)
    v1, j1 = ops.lbs(bd[:130].contiguous(), rd[:130].contiguous(), model, use_mfma=1)
    v0, j0 = ops.lbs(bd[:100].contiguous(), rd[:100].contiguous(), model, use_mfma=1)
    assert torch.equal(v4[:130], v1) and torch.equal(j4[:130], j1)
    assert torch.equal(v1[:100], v0) and torch.equal(j1[:100], j0)
    vt, _ = ops.lbs(bd[B4 - 70:].contiguous(), rd[B4 - 70:].contiguous(), model, use_mfma=1)      # other row offsets inside the tiles
    assert torch.equal(v4[B4 - 70:], vt)


class _Ctx:
    """Stands in for autograd's context: _LbsFn.forward / .backward called directly, so that a cotangent can be None (autograd itself
    materialises the cotangent of an unused output as zeros and never takes those paths)."""

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


@gpu
@pytest.mark.parametrize("use_mfma", [0, 1])
@pytest.mark.parametrize("keep", [None, 3])
def test_cotangent_on_one_output_only(keep, use_mfma):
    """Loss on verts only and on joints only, through autograd (zeros for the unused output) and with the cotangent None
    (grad_joints == nullptr in the library; zeros made by ops.py for verts).  Under a joints-only loss the fingertip joints' blocks
    of g_rot are exactly zero, and exempt from the measure's floor only in that they are compared as == 0."""
    from followmyhold_amd import ops
    name = "a_dense" if keep is None else "a_keep3"
    m, (b, r, gv, gj), _ = case(name)
    model = _device_model(778, keep)
    leaves = list(G.LEAVES)
    for which, cv, cj in (("verts only", gv, None), ("joints only", None, gj)):
        ref = G.lbs(b, r, m, cv, cj)
        got = _kernel(model, b, r, cv, cj, use_mfma)
        e = G.measure(got, ref)
        _report(f"{name} use_mfma {use_mfma}, {which}, autograd", e)
        assert _within(e), e
        ctx = _Ctx()
        bd, rd = torch.tensor(b).cuda(), torch.tensor(r).cuda()
        verts, joints = ops._LbsFn.forward(ctx, bd, rd, model, use_mfma)
        gb, gr, _, _ = ops._LbsFn.backward(ctx, None if cv is None else torch.tensor(cv).cuda(), None if cj is None else torch.tensor(cj).cuda())
        raw = tuple(t.cpu().numpy() for t in (verts, joints, gb, gr))
        e = G.measure(raw, ref)
        _report(f"{name} use_mfma {use_mfma}, {which}, cotangent None", e)
        assert _within(e), e
        if cv is None:
            assert (ref[3][:, leaves] == 0).all()
            assert (got[3][:, leaves] == 0).all() and (raw[3][:, leaves] == 0).all()


@gpu
@pytest.mark.parametrize("keep", [None, 3])
def test_two_backward_calls_from_one_forward(keep):
    """k_lbs_bwd_posefeat overwrites the forward's pose-feature slot of the workspace and g_A is re-zeroed: a second backward from the
    same forward must be as good as the first (not bitwise equal: g_A goes through float atomics)."""
    from followmyhold_amd import ops
    name = "a_dense" if keep is None else "a_keep3"
    _, (b, r, gv, gj), ref = case(name)
    bd, rd = torch.tensor(b).cuda().requires_grad_(True), torch.tensor(r).cuda().requires_grad_(True)
    verts, joints = ops.lbs(bd, rd, _device_model(778, keep), use_mfma=1)
    loss = (verts * torch.tensor(gv).cuda()).sum() + (joints * torch.tensor(gj).cuda()).sum()
    for n in (1, 2):
        bd.grad = rd.grad = None
        loss.backward(retain_graph=True)
        e = G.measure((None, None, bd.grad.cpu().numpy(), rd.grad.cpu().numpy()), ref)
        _report(f"{name}: backward {n} of 2", e)
        assert _within(e), e
    # ... and with other cotangents in between: nothing of the first backward may leak into the second
    (verts.sum() - joints.sum()).backward(retain_graph=True)
    bd.grad = rd.grad = None
    loss.backward()
    e = G.measure((None, None, bd.grad.cpu().numpy(), rd.grad.cpu().numpy()), ref)
    _report(f"{name}: backward after a backward with other cotangents", e)
    assert _within(e), e


@gpu
def test_float64_betas_and_non_contiguous_rotations():
    """The caller's dtype and layout: float64 betas and a non-contiguous rot_mats get gradients of their own dtype and shape."""
    from followmyhold_amd import ops
    _, (b, r, gv, gj), ref = case("a_keep3")
    bd = torch.tensor(b).double().cuda().requires_grad_(True)
    rd = torch.tensor(np.ascontiguousarray(r.transpose(1, 0, 2, 3))).cuda().permute(1, 0, 2, 3).requires_grad_(True)
    assert not rd.is_contiguous() and rd.is_leaf
    verts, joints = ops.lbs(bd, rd, _device_model(778, 3), use_mfma=-1)
    ((verts * torch.tensor(gv).cuda()).sum() + (joints * torch.tensor(gj).cuda()).sum()).backward()
    assert bd.grad.dtype == torch.float64 and bd.grad.shape == (3, 10)
    assert rd.grad.dtype == torch.float32 and rd.grad.shape == (3, 16, 3, 3)
    e = G.measure(tuple(t.detach().cpu().numpy() for t in (verts, joints, bd.grad, rd.grad)), ref)
    _report("a_keep3, float64 betas, non-contiguous rot", e)
    assert _within(e), e


@gpu
@pytest.mark.parametrize("use_mfma", [0, 1])
def test_known_answers_kernel(use_mfma):
    """The closed-form answers of test_known_answers_referee within the forward bound; the leaf-joint gradient of sum(joints) == 0."""
    from followmyhold_amd import ops
    for name, m, betas, rot, v_exp, j_exp in _known_answers():
        v, j = ops.lbs(torch.tensor(betas).cuda(), torch.tensor(rot).cuda(), _lbs_model(m), use_mfma=use_mfma)
        e = G.measure((v.cpu().numpy(), j.cpu().numpy(), None, None), (v_exp, j_exp, None, None))
        _report(f"known answer {name}, use_mfma {use_mfma}", e)
        assert _within(e), (name, e)
    _, (b, r, _, _), _ = case("a_keep3")
    bd, rd = torch.tensor(b).cuda().requires_grad_(True), torch.tensor(r).cuda().requires_grad_(True)
    _, joints = ops.lbs(bd, rd, _device_model(778, 3), use_mfma=use_mfma)
    joints.sum().backward()
    gr = rd.grad.cpu().numpy()
    assert (gr[:, list(G.LEAVES)] == 0).all() and all(np.abs(gr[:, i]).max() > 0 for i in range(16) if i not in G.LEAVES)
