"""k_geo_attn, k_geo_attn_bwd and k_geo_attn_dq (csrc/foho_geo.hip) over the full range of fp16 logits, against the float64 referee of
tests/attn_ref64.py.

The other attention tests draw q, k and v from randn: scores within +-45 log2 units, a score near the row's maximum among the first 32
keys.  Here the scores follow ten profiles (attn_ref64.CASES) aimed at the online softmax itself -- the running maximum that the first
unit of 32 keys sets, the rescale that is deferred until a score exceeds it by 2^6 -- at scores between -300 and +1000 log2 units: what
LayerNorm gains and outlier channels produce and unit Gaussians do not.  The tolerances are derived, next to each assertion, from the
roundings the kernels document, eps = 2^-11 relative to the componentwise magnitude bounds of `attn_ref64.bounds`; no other fp16
implementation is a yardstick.  Every test prints its largest err / (eps B) per output (-s shows them).

Measured on an MI355X, the largest figure over the shapes of an entry point.  O and the gradients: err / (eps B), bounds 3 and 8; nlse and
lse_nat: err in units of 2^-23 max(1, |S|), bound 8; dV `raw`: without the fp16-underflow term of `_assert_grads`, where that matters.

  case                     geo O   sdpa O   nlse   lse_nat   dV      dQ      dK      raw
  cold_first_unit          0.571   0.412    0.119  0.090     0.487   0.079   0.060              (NaN in every row before the fix)
  cold_first_tile          0.557   0.519    0.147  0.097     0.529   0.126   0.062              (NaN in every row before the fix)
  cold_one_query_block     0.659   0.439    0.916  0.646     0.729   0.094   0.135              (NaN in rows 32..63 of every wave before)
  late_dominator           0.000   0.000    1.535  1.195     0.243   0.000   0.000   dK 645     (dK_ref is 1e-71 throughout: the kernel's 0)
  stairs_below_threshold   0.767   0.462    2.272  1.733     0.415   0.057   0.063
  stairs_above_threshold   0.794   0.824    0.877  0.859     0.471   0.059   0.059   dV 771
  one_hot_lane             0.553   0.829    0.562  0.677     1.713   0.080   0.500   dV 50.8
  uniform                  0.284   0.169    4.470  4.522     0.227   0.021   0.074
  high_plateau             1.506   1.223    0.525  0.580     0.353   0.086   0.056   dV 386
  wide_spread              1.857   1.722    1.310  0.952     0.469   0.123   0.048
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_ref64 as R  # noqa: E402

gpu = pytest.mark.gpu

EPS = 2.0 ** -11                                                  # half an ulp of fp16, relative
GEO_SHAPES = [(70, 64, 2),                                        # M, L, heads: one key tile, both query blocks, ragged rows
              (300, 192, 3),                                      # blockIdx % heads, a second workgroup
              (96, 128, 8)]                                       # the XCD head mapping
SDPA_SHAPES = [(2, 2, 70, 128), (1, 8, 300, 256)]                 # B, H, M, L; the second also in the interleaved q | k | v layout
REPEATED = ("cold_first_unit", "stairs_above_threshold")          # bitwise repeatability is asserted on these
GEO_PARAMS = [(M, L, h, c) for (M, L, h) in GEO_SHAPES for c in R.CASES if not (c == "cold_first_tile" and L < 128)]
SDPA_PARAMS = [(B, H, M, L, c) for (B, H, M, L) in SDPA_SHAPES for c in R.CASES]


@functools.lru_cache(maxsize=None)
def _case(case, heads, M, L, unscaled_q):
    """The operands of a case and the referee's forward on them; computed once, shared, never written to."""
    op = R.build(case, heads, M, L, unscaled_q=unscaled_q)
    op["S"], op["P"], op["O"], op["lse2"] = R.forward(op["Qs"], op["K"], op["V"])
    for a in op.values():
        a.setflags(write=False)
    return op


def _ratio(err, B, floor):
    """Largest (err - floor)+ / (eps B): `err <= k eps B + floor` everywhere is `_ratio <= k`."""
    over = np.maximum(err - floor, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(over > 0.0, over / (EPS * B), 0.0)
    return float(r.max())


# ---------------------------------------------------------------- the referee and the cases, without a GPU
def test_referee_forward_is_float64_softmax_attention():
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(3, n, 64, generator=g, dtype=torch.float64) for n in (37, 96, 96))
    S, P, O, lse2 = R.forward((q * (R.LOG2E / 8.0)).numpy(), k.numpy(), v.numpy())
    s = q @ k.transpose(-1, -2) / 8.0
    assert np.abs(P - torch.softmax(s, dim=-1).numpy()).max() <= 1e-12
    assert np.abs(O - (torch.softmax(s, dim=-1) @ v).numpy()).max() <= 1e-12
    assert np.abs(S - s.numpy() * R.LOG2E).max() <= 1e-12
    assert np.abs(lse2 - torch.logsumexp(s, dim=-1).numpy() * R.LOG2E).max() <= 1e-12


def test_referee_backward_is_float64_autograd():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, n, 64, generator=g, dtype=torch.float64).requires_grad_(True) for n in (41, 64, 64))
    go = torch.randn(2, 41, 64, generator=g, dtype=torch.float64)
    out = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v
    out.backward(go)
    Qs = (q.detach() * (R.LOG2E / 8.0)).numpy()
    dQ, dK, dV, dS = R.backward(Qs, k.detach().numpy(), v.detach().numpy(), go.numpy(), out.detach().numpy())
    for got, want in ((dQ, q.grad), (dK, k.grad), (dV, v.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-10
    # the bounds are bounds: |g| <= B_g componentwise (same products, absolute values)
    B = R.bounds(Qs, k.detach().numpy(), v.detach().numpy(), go.numpy(), out.detach().numpy())
    O = R.forward(Qs, k.detach().numpy(), v.detach().numpy())[2]
    for got, name in ((O, "O"), (dV, "dV"), (dS, "dS"), (dQ, "dQ"), (dK, "dK")):
        assert (np.abs(got) <= B[name] * (1 + 1e-12)).all(), name


def test_referee_known_answers():
    rng = np.random.default_rng(5)
    L = 96
    V = rng.standard_normal((L, 64))
    Qs = rng.standard_normal((7, 64))
    k0 = rng.standard_normal(64)
    # identical keys: every row attends uniformly, O = mean(V), lse2 = s + log2 L
    S, P, O, lse2 = R.forward(Qs, np.tile(k0, (L, 1)), V)
    assert np.abs(O - V.mean(axis=0)).max() <= 1e-13 and np.abs(lse2 - (Qs @ k0 + np.log2(L))).max() <= 1e-12
    # one key 300 log2 units above all others: O = V[that key], exactly (2^-300 of the rest is below half an ulp of float64)
    w = np.ones(64)
    K = 0.01 * rng.standard_normal((L, 64))
    K -= (K @ w)[:, None] * w / 64.0
    K[17] += 40.0 / 8.0 * w
    Qs = 8.0 / 8.0 * w + 0.0 * Qs
    S, P, O, lse2 = R.forward(Qs, K, V)
    assert (S[:, 17] - np.delete(S, 17, axis=1).max(axis=1)).min() >= 300.0
    assert np.array_equal(O, np.tile(V[17], (7, 1))) and np.abs(lse2 - S[:, 17]).max() == 0.0
    # the fault the cold-start cases aim at is one of float32, not of the mathematics: 2^150 overflows, 2^-150 underflows
    with np.errstate(all="ignore"):
        assert np.isinf(np.exp2(np.float32(150.0))) and np.exp2(np.float32(-150.0)) == 0.0 and np.isnan(np.float32(0.0) * np.exp2(np.float32(150.0)))


def test_qs_as_loaded_is_one_float32_product_rounded_to_fp16():
    q = np.array([1.0, -3.0, 22.0, 0.001, 65504.0], dtype=np.float16)
    got = R.qs_as_loaded(q)
    assert got.dtype == np.float16
    want = [np.float16(np.float32(x) * np.float32(1.4426950408889634 * 0.125)) for x in q]
    assert np.array_equal(got, np.array(want, dtype=np.float16))


@pytest.mark.parametrize("entry,heads,M,L,case", [("geo", h, M, L, c) for (M, L, h, c) in GEO_PARAMS] + [("sdpa", B * H, M, L, c) for (B, H, M, L, c) in SDPA_PARAMS])
def test_cases_are_fp16_and_their_realised_scores_have_the_named_property(entry, heads, M, L, case):
    """A condition, not a measurement: a case whose rounded operands lose its point fails HERE, without a GPU."""
    op = _case(case, heads, M, L, entry == "sdpa")
    for name in ("Qs", "K", "V", "dO") + (("q",) if entry == "sdpa" else ()):
        assert op[name].dtype == np.float16 and np.isfinite(op[name]).all(), name
    if entry == "sdpa":
        assert np.array_equal(R.qs_as_loaded(op["q"]), op["Qs"])
    R.check_property(case, op["S"])                                # S: the referee's scores of the ROUNDED values
    assert np.isfinite(op["O"]).all() and np.isfinite(op["lse2"]).all()
    if case == "uniform":
        assert np.abs(op["O"] - op["V"].astype(np.float64).mean(axis=1, keepdims=True)).max() <= 1e-12
        assert np.abs(op["lse2"] - (op["S"][..., 0] + np.log2(L))).max() <= 1e-12
    if case == "late_dominator":
        assert np.abs(op["O"] - op["V"][:, -1:].astype(np.float64)).max() <= 1e-30


def test_lazy_schedule_follows_the_kernels_rule():
    S = np.zeros((1, 4 * R.UNIT))
    S[0, 40], S[0, 70], S[0, 100] = 5.0, 9.0, 14.0                 # +5: stays; +9: raises to 9; 14 - 9 = 5: stays
    first, rel = R.lazy_schedule(S)
    assert first[0] == 0.0 and rel[0].tolist() == [0.0, 5.0, 9.0, 5.0]


# ---------------------------------------------------------------- the assertions
def _assert_O(tag, O16, op, B_O):
    got = O16.astype(np.float64)
    assert np.isfinite(got).all(), f"{tag}: O is not finite ({np.isnan(got).sum()} NaN, {np.isinf(got).sum()} inf of {got.size})"
    err = np.abs(got - op["O"])
    r = _ratio(err, B_O, 2.0 ** -24)
    print(f"{tag}: O err / (eps B) {r:.3f}")
    # |O - O_ref| <= 3 eps B_O + 2^-24, B_O = P |V|.  P is rounded to fp16 for the matrix instruction while the denominator is summed from
    # the unrounded fp32 values: numerator only, eps B_O.  The store rounds O to fp16: eps |O| <= eps B_O.  The third eps is for the fp32
    # accumulation (64 terms per score, L per output; 2^-24 each, not all one way) and v_exp_f32 (1 ulp on a score kept to 2^-24 relative:
    # at |S| = 1000 that is 2^-14 absolute, 2^-14 ln 2 relative on P).  2^-24: the smallest fp16 subnormal, for outputs that round to 0.
    assert r <= 3.0, f"{tag}: O exceeds 3 eps B_O + 2^-24 by the factor {r / 3.0:.2f}"


def _assert_lse(tag, nlse, lse_nat, op, M):
    """nlse (heads, Mpad) and lse_nat (heads, M) as float64."""
    # fp32 quantities at the magnitude of the scores: -(running max), accumulated in fp32 from differences of fp32 scores, and log2 of a sum
    # in [1, 64 L]; the scores themselves carry 64 roundings of 2^-24 each way, at the magnitude of their partial sums.  8 ulp of 2^-23 at
    # max(1, max |S|), the maximum over the head's scores -- and per row no more than that row's own arithmetic can reach, max_j |Qs_i|.|K_j|
    # (>= |S_ij|: a row of small scores among large ones is held to ITS magnitude.  max_j |S_ij| itself is too small a scale: the 64 products
    # of an ordinary row of cold_one_query_block sum to 14 in magnitude and cancel to |S| <= 4.4; measured 9.8 ulp of THAT, 3 of the former.)
    Qa, Ka = np.abs(op["Qs"].astype(np.float64)), np.abs(op["K"].astype(np.float64))
    reach = (Qa @ np.swapaxes(Ka, -1, -2)).max(axis=-1)
    scale = np.maximum(1.0, np.minimum(reach, np.abs(op["S"]).max(axis=(-1, -2))[:, None]))
    tol = 8.0 * 2.0 ** -23 * scale
    assert np.isfinite(nlse[:, :M]).all() and np.isfinite(lse_nat).all(), f"{tag}: lse is not finite"
    e2, en = np.abs(nlse[:, :M] + op["lse2"]), np.abs(lse_nat - op["lse2"] * R.LN2)
    print(f"{tag}: nlse err / (2^-23 max(1, |S|)) {float((e2 / tol).max()) * 8:.3f}  lse_nat {float((en / tol).max()) * 8:.3f}")
    assert (e2 <= tol).all() and (en <= tol).all(), f"{tag}: lse off by {float((e2 / tol).max()) * 8:.2f} / {float((en / tol).max()) * 8:.2f} x 2^-23 max(1, |S|)"
    assert np.isneginf(nlse[:, M:]).all(), f"{tag}: the pad rows of nlse must be -inf"       # (P = 0 for them in the backward)


def _grad_refs_and_bounds(op, O16):
    """-> {name: (g_ref, B_g, floor, U)} for dV, dQ, dK: the referee's gradients and the three terms of `_assert_grads`' tolerance
    8 eps B_g + floor + U (tests/test_vae_stages.py carries the same tolerance through the qk_norm backward)."""
    dQ, dK, dV, _ = R.backward(op["Qs"], op["K"], op["V"], op["dO"], O16)
    B = R.bounds(op["Qs"], op["K"], op["V"], op["dO"], O16)
    # fp16 UNDERFLOW, the rounding the relative bound below does not contain: below 2^-14 fp16 is subnormal, its rounding error is half a
    # quantum of 2^-24 whatever the value, and below 2^-25 a value becomes 0.  P and dS are fp16 operands of the matrix instructions, so
    # every term of a sum carries up to 2^-25 |partner|: dV_jd = sum_i P_ij dO_id -> 2^-25 sum_i |dO_id|; dK_jd = ln 2 sum_i dS_ij Qs_id ->
    # 2^-25 ln 2 sum_i |Qs_id|; dQ_id = sum_j dS_ij K_jd / 8 -> 2^-25 sum_j |K_jd| / 8; and the stored result another 2^-25.  At most 1e-5
    # on gradients of order 1.  It shows where a key's P is 2^-15 .. 2^-25 in EVERY row (the staircases, the plateau, the hot lane: rows
    # with the same s_i): there eps B_g is as small as the term itself; measured without it, up to 770 eps B_dV (printed as `raw`).
    a64 = lambda n: np.abs(op[n].astype(np.float64))
    U = {"dV": 2.0 ** -25 * (a64("dO").sum(axis=1, keepdims=True) + 1.0), "dK": 2.0 ** -25 * (R.LN2 * a64("Qs").sum(axis=1, keepdims=True) + 1.0),
         "dQ": 2.0 ** -25 * (a64("K").sum(axis=1, keepdims=True) / 8.0 + 1.0)}
    return {name: (ref, B[name], 2.0 ** -24 * np.abs(ref).max(), U[name]) for name, ref in (("dV", dV), ("dQ", dQ), ("dK", dK))}


def _assert_grads(tag, grads, op, O16):
    worst, raw = {}, {}
    for name, (ref, B, floor, U) in _grad_refs_and_bounds(op, O16).items():
        got = grads[name].astype(np.float64)
        assert np.isfinite(got).all(), f"{tag}: {name} is not finite ({np.isnan(got).sum()} NaN of {got.size})"
        worst[name], raw[name] = _ratio(np.abs(got - ref), B, floor + U), _ratio(np.abs(got - ref), B, floor)
    print(f"{tag}: " + "  ".join(f"{k} err / (eps B) {v:.3f} (raw {raw[k]:.3f})" for k, v in worst.items()))
    # |g - g_ref| <= 8 eps B_g + 2^-24 max |g_ref| (+ the underflow term above).  Five fp16 roundings lie between the operands and a stored
    # gradient: P (operand of dV = P^T dO), dS (operand of dQ and dK), O inside delta = rowsum(dO O) (the referee is GIVEN the stored O;
    # what is left is delta's own rounding), the rescaled / transposed operand copies (Qs rounded once; dO^T, K^T exact), the fp16 store of
    # the result -- summed linearly, 5 eps B.  The other 3 eps: fp32 accumulation over at most 300 terms (2^-24 each, growing like the root
    # of their number when they do not all point one way) and v_exp_f32 on scores kept in fp32 (as for O).
    for name, r in worst.items():
        assert r <= 8.0, f"{tag}: {name} exceeds 8 eps B + 2^-24 max|g| + underflow by the factor {r / 8.0:.2f}"


# ---------------------------------------------------------------- foho_geo_attention: the decoder's entry point, Q pre-scaled
def _geo_run(lib, qs, kv, M, L, heads):
    W = heads * 64
    O = torch.full((M, W), float("nan"), dtype=torch.float16, device="cuda")
    vt = torch.empty(W * L, dtype=torch.float16, device="cuda")
    rc = lib.foho_geo_attention(qs.data_ptr(), kv.data_ptr(), vt.data_ptr(), O.data_ptr(), M, L, heads, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.foho_geo_last_error()
    torch.cuda.synchronize()
    return O


@gpu
@pytest.mark.parametrize("M,L,heads,case", GEO_PARAMS)
def test_geo_attention_over_the_score_range(M, L, heads, case):
    from followmyhold_amd import _lib
    lib = _lib.lib()
    op = _case(case, heads, M, L, False)
    W = heads * 64
    rows = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(a.shape[1], W))     # (heads, n, 64) -> (n, heads * 64)
    qs = rows(op["Qs"]).cuda()
    kv = torch.cat([rows(op["K"]), rows(op["V"])], dim=1).contiguous().cuda()                               # the KV projection's layout: K | V
    O = _geo_run(lib, qs, kv, M, L, heads)
    O16 = O.cpu().numpy().reshape(M, heads, 64).transpose(1, 0, 2)
    tag = f"geo M={M} L={L} heads={heads} {case}"
    _assert_O(tag, O16, op, R.bounds(op["Qs"], op["K"], op["V"])["O"])
    if case == "late_dominator":        # alpha underflows to 0, P = 1 for the last key alone: V[last], at most rounded once more
        assert (np.abs(O16.astype(np.float64) - op["V"][:, -1:].astype(np.float64)) <= EPS * np.abs(op["V"][:, -1:].astype(np.float64))).all()
    if case in REPEATED:
        assert torch.equal(_geo_run(lib, qs, kv, M, L, heads), O)


# ---------------------------------------------------------------- sdpa.attention: foho_sdpa_fwd (scales q on load) and the HIP backward
def _bhnd(a, B, H):
    return torch.from_numpy(a.reshape(B, H, a.shape[1], 64).copy()).cuda()


def _sdpa_fwd_direct(q, k, v):
    """foho_sdpa_fwd as sdpa._HipSdpaFn.forward calls it, with BOTH log-sum-exp outputs -> out (B, H, M, 64), nlse (B, Mpad, H), lse_nat (B, H, M)."""
    from followmyhold_amd import _lib as L, sdpa
    lib = L.lib()
    B, H, M, _ = q.shape
    Lk = k.shape[2]
    assert sdpa._in_place(q, k, v)
    out = torch.full((B, M, H * 64), float("nan"), dtype=torch.float16, device=q.device)
    nlse = torch.full((B, (M + 63) // 64 * 64, H), float("nan"), dtype=torch.float32, device=q.device)
    lse = torch.full((B, H, M), float("nan"), dtype=torch.float32, device=q.device)
    ws = sdpa._workspace(lib, q.device, M, Lk, H)
    d = sdpa._desc(q, k)
    rc = lib.foho_sdpa_fwd(ctypes.byref(d), L._p(q), L._p(k), L._p(v), L._p(out), L._p(nlse), L._p(lse), L._p(ws), ws.numel(), L._stream(q.device))
    L.geo_check(rc, "foho_sdpa_fwd")
    torch.cuda.synchronize()
    return out.view(B, M, H, 64).transpose(1, 2), nlse, lse


def _sdpa_fwd_bwd(q, k, v, go, leaves=None):
    """sdpa.attention and its backward -> out, [grads of `leaves` (default: q, k, v)]."""
    from followmyhold_amd import sdpa
    out = sdpa.attention(q, k, v)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in (leaves or (q, k, v))]


@gpu
@pytest.mark.parametrize("B,H,M,L,case", SDPA_PARAMS)
def test_sdpa_forward_and_hip_backward_over_the_score_range(B, H, M, L, case, monkeypatch):
    from followmyhold_amd import sdpa
    monkeypatch.setattr(sdpa, "backward_route", "hip")              # this package's kernels; the torch route is not ours
    op = _case(case, B * H, M, L, True)
    q, k, v, go = (_bhnd(op[n], B, H) for n in ("q", "K", "V", "dO"))
    tag = f"sdpa B={B} H={H} M={M} L={L} {case}"
    out_d, nlse, lse_nat = _sdpa_fwd_direct(q, k, v)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out, (gq, gk, gv) = _sdpa_fwd_bwd(*leaves, go)
    np_h = lambda t: t.contiguous().cpu().numpy().reshape(B * H, t.shape[2], 64)
    O16 = np_h(out)
    _assert_O(tag, O16, op, R.bounds(op["Qs"], op["K"], op["V"])["O"])
    assert torch.equal(out, out_d)
    Mp = nlse.shape[1]
    _assert_lse(tag, nlse.permute(0, 2, 1).reshape(B * H, Mp).double().cpu().numpy(), lse_nat.reshape(B * H, M).double().cpu().numpy(), op, M)
    _assert_grads(tag, {"dQ": np_h(gq), "dK": np_h(gk), "dV": np_h(gv)}, op, O16)
    if case in REPEATED:
        again = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out2, g2 = _sdpa_fwd_bwd(*again, go)
        assert torch.equal(out2, out) and all(torch.equal(a, b) for a, b in zip(g2, (gq, gk, gv)))
    if B == 1 and H == 8:
        # hy3dgen's c_qkv layout, what vae_transformer hands over: rows of H x [q | k | v]; the M queries and the L keys are the first rows
        # of one buffer (head stride 192, row stride 192 H) -- same numbers, same bits
        N = max(M, L)
        qkv = torch.zeros(1, N, H, 192, dtype=torch.float16, device="cuda")
        qkv[:, :M, :, 0:64], qkv[:, :L, :, 64:128], qkv[:, :L, :, 128:192] = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
        qkv.requires_grad_(True)
        q4, k4, v4 = qkv[:, :M, :, 0:64].transpose(1, 2), qkv[:, :L, :, 64:128].transpose(1, 2), qkv[:, :L, :, 128:192].transpose(1, 2)
        assert q4.stride(1) == 192 and sdpa._in_place(q4, k4, v4)
        out4, (g4,) = _sdpa_fwd_bwd(q4, k4, v4, go, leaves=(qkv,))
        assert torch.equal(out4, out)
        assert torch.equal(g4[:, :M, :, 0:64].transpose(1, 2), gq) and torch.equal(g4[:, :L, :, 64:128].transpose(1, 2), gk)
        assert torch.equal(g4[:, :L, :, 128:192].transpose(1, 2), gv)
