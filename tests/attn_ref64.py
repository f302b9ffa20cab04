"""A float64 referee for head-dimension-64 attention (k_geo_attn, k_geo_attn_bwd, k_geo_attn_dq in csrc/foho_geo.hip), CPU only, numpy
only: nothing of the package is imported.

The kernels work in log2 units: Qs = q log2(e) / 8 rounded to fp16 (by the caller of foho_geo_attention, by the load of foho_sdpa_fwd --
`qs_as_loaded`), S = Qs K^T, P = 2^(S - rowmax) / sum, O = P V, lse2 = rowmax + log2 sum.  The referee evaluates exactly that from the
fp16 values the kernels read, per head: arrays are (..., M, 64) for Qs / dO / O and (..., L, 64) for K / V, leading axes (heads, batch)
broadcast through.

Backward, for the cotangent dO of O and with delta formed from the fp16 output the forward STORED (as k_geo_delta forms it):

  dV = P^T dO        dP = dO V^T        delta = rowsum(dO * O16)        dS = P * (dP - delta)      (w.r.t. the NATURAL-log scores q k^T / 8)
  dQ = dS K / 8      dK = dS^T q / 8,  q / 8 = Qs ln 2                                             (w.r.t. the unscaled q and k)

`bounds` evaluates the same products with absolute values: the componentwise magnitudes that every rounding on the kernels' path is
relative to (tests/test_attention_range.py builds its tolerances from them).

The second half builds the score profiles of tests/test_attention_range.py and states, per profile, the property of the REALISED scores
(the referee's S of the fp16-rounded operands) that the profile is named for."""
import numpy as np

LN2 = float(np.log(2.0))
LOG2E = 1.4426950408889634
UNIT = 32                       # keys per unit of k_geo_attn's online softmax
THR = 6.0                       # RESCALE_THR of csrc/foho_geo.hip, log2 units


def _T(a):
    return np.swapaxes(a, -1, -2)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------- the referee
def qs_as_loaded(q):
    """The one rounding foho_sdpa_fwd applies as it loads q: (h16)((float)q * SDPA_QSCALE), SDPA_QSCALE = log2(e) / 8 in float32."""
    return (np.asarray(q, dtype=np.float16).astype(np.float32) * np.float32(LOG2E * 0.125)).astype(np.float16)


def forward(Qs, K, V):
    """-> S (.., M, L), P (.., M, L), O (.., M, 64), lse2 (.., M): float64."""
    Qs, K, V = _f64(Qs), _f64(K), _f64(V)
    S = Qs @ _T(K)
    m = S.max(axis=-1, keepdims=True)
    E = np.exp2(S - m)
    sm = E.sum(axis=-1, keepdims=True)
    P = E / sm
    return S, P, P @ V, (m + np.log2(sm))[..., 0]


def backward(Qs, K, V, dO, O16):
    """-> dQ (.., M, 64), dK (.., L, 64), dV (.., L, 64), dS (.., M, L): float64; dQ / dK w.r.t. the unscaled q / k of softmax(q k^T / 8) v."""
    Qs, K, V, dO, O16 = _f64(Qs), _f64(K), _f64(V), _f64(dO), _f64(O16)
    P = forward(Qs, K, V)[1]
    dV = _T(P) @ dO
    delta = (dO * O16).sum(axis=-1, keepdims=True)
    dS = P * (dO @ _T(V) - delta)
    return dS @ K / 8.0, _T(dS) @ Qs * LN2, dV, dS


def bounds(Qs, K, V, dO=None, O16=None):
    """The magnitudes the roundings are relative to: {"O": P |V|} and, with dO and O16, {"dV": P^T |dO|, "dS": P * (|dO| |V|^T +
    rowsum(|dO| * |O16|)), "dQ": B_dS |K| / 8, "dK": B_dS^T |q| / 8} (|q| / 8 = |Qs| ln 2)."""
    Qs, K, V = _f64(Qs), _f64(K), _f64(V)
    P = forward(Qs, K, V)[1]
    B = {"O": P @ np.abs(V)}
    if dO is not None:
        dO, O16 = np.abs(_f64(dO)), np.abs(_f64(O16))
        B["dV"] = _T(P) @ dO
        B["dS"] = P * (dO @ _T(np.abs(V)) + (dO * O16).sum(axis=-1, keepdims=True))
        B["dQ"] = B["dS"] @ np.abs(K) / 8.0
        B["dK"] = _T(B["dS"]) @ np.abs(Qs) * LN2
    return B


# ---------------------------------------------------------------- the kernel's schedule of running maxima, on the referee's scores
def lazy_schedule(S):
    """k_geo_attn's running maximum, row by row, on float64 scores S (.., M, L): the first unit of 32 keys SETS it to the unit's maximum,
    a later unit raises it to its own maximum when that exceeds it by more than THR.  -> first (.., M): the first unit's maximum;
    rel (.., M, L / 32): every unit's maximum minus the running maximum it met (unit 0: zero).  (In the kernel a unit rescales when ANY of
    its 32 rows exceeds the threshold and the other rows then take max(tm, 0); a row whose own `rel` never exceeds THR keeps its running
    maximum either way, which is all the profiles below rely on.)"""
    S = _f64(S)
    um = S.reshape(S.shape[:-1] + (S.shape[-1] // UNIT, UNIT)).max(axis=-1)
    run = um[..., 0].copy()
    rel = np.zeros_like(um)
    for u in range(1, um.shape[-1]):
        rel[..., u] = um[..., u] - run
        run = np.where(rel[..., u] > THR, um[..., u], run)
    return um[..., 0], rel


# ---------------------------------------------------------------- score profiles
CASES = ("cold_first_unit", "cold_first_tile", "cold_one_query_block", "late_dominator", "stairs_below_threshold", "stairs_above_threshold",
         "one_hot_lane", "uniform", "high_plateau", "wide_spread")
NOISE = 0.05
HOT_ROW = 13                    # one_hot_lane: the row of every wave (64 queries) that jumps


def _w():
    return np.where(np.arange(64) % 3 == 0, -1.0, 1.0)        # a fixed +-1 vector: |w|^2 = 64


def _noise(rng, shape):
    """0.05 randn, with its component along w taken out: the cross terms (s/8) w.eta and (c/8) w.eps would otherwise move the base score
    s_i c_j by 0.05 sqrt(s^2 + c^2) -- +-1 at the staircases' 5.5 / 6.5, which have 0.5 to spare.  What stays is eps.eta, sigma 0.02."""
    w = _w()
    n = NOISE * rng.standard_normal(shape)
    return n - (n @ w)[..., None] * w / 64.0


def profile(case, heads, M, L, seed=0):
    """-> s (heads, M), c (heads, L): the base scores s_i c_j of the case, in log2 units."""
    rng = np.random.default_rng([seed, CASES.index(case), heads, M, L])
    nu = L // UNIT
    row, unit = np.arange(M) % 64, np.arange(L) // UNIT
    U = lambda lo, hi, n: rng.uniform(lo, hi, (heads, n))
    if case in ("cold_first_unit", "cold_first_tile"):
        ncold = UNIT if case == "cold_first_unit" else 2 * UNIT
        assert L >= 2 * ncold
        s, c = U(4.0, 6.0, M), U(-0.25, 0.25, L)
        c[:, :ncold] = U(-44.0, -40.0, ncold)                  # scores -264 .. -160
    elif case == "cold_one_query_block":
        s, c = np.where(row >= 32, U(4.0, 6.0, M), U(-0.1, 0.1, M)), U(-0.25, 0.25, L)
        c[:, :UNIT] = U(-44.0, -40.0, UNIT)
    elif case == "late_dominator":
        s, c = U(4.0, 6.0, M), U(-1.0, 1.0, L)
        c[:, -1] = 60.0                                        # 240 .. 360 against |s c| <= 6
    elif case in ("stairs_below_threshold", "stairs_above_threshold"):
        step = 5.5 if case == "stairs_below_threshold" else 6.5
        level, run = np.zeros(nu), 0.0
        for u in range(1, nu):                                 # every unit `step` above the running maximum it meets in the kernel
            level[u] = run + step
            run = level[u] if step > THR else run
        s = np.full((heads, M), 2.0)
        c = (level[unit] - U(1.0, 4.0, L)) / 2.0
        c[:, 7::UNIT] = level / 2.0                            # one key per unit carries the unit's maximum
    elif case == "one_hot_lane":
        s = np.where(row == HOT_ROW, 4.0, -1.0) * np.ones((heads, 1))
        c = U(-0.5, 0.0, L)
        c[:, unit == 1] = U(13.5, 14.0, UNIT)                  # the hot row: +54 .. +56; its neighbours: -14
        if nu > 2:
            c[:, unit == nu - 1] = U(27.5, 28.0, UNIT)         # ... and once more, in the last unit
    elif case == "uniform":
        s, c = U(-3.0, 3.0, M), np.full((heads, L), 2.0)
    elif case == "high_plateau":
        s, c = U(30.5, 31.5, M), U(29.8, 31.5, L)              # 908.9 .. 992.25
    elif case == "wide_spread":
        s, c = rng.choice([-1.0, 1.0], (heads, M)) * U(15.0, 17.2, M), U(-17.2, 17.2, L)
        c[:, 3], c[:, -5] = 17.2, -17.2
    else:
        raise ValueError(case)
    return s, c


def build(case, heads, M, L, seed=0, unscaled_q=False):
    """The operands of one case, per head, fp16: Qs (heads, M, 64), K, V (heads, L, 64), dO (heads, M, 64).
    unscaled_q: also q, the fp16 values whose `qs_as_loaded` is the returned Qs (for foho_sdpa_fwd, which scales on load)."""
    s, c = profile(case, heads, M, L, seed)
    rng = np.random.default_rng([seed + 1, CASES.index(case), heads, M, L])
    w = _w()
    eps, eta = _noise(rng, (heads, M, 64)), _noise(rng, (heads, L, 64))
    if case == "uniform":
        eta[:] = eta[:, :1]                                    # all keys EQUAL
    Qs = s[..., None] / 8.0 * w + eps
    K = (c[..., None] / 8.0 * w + eta).astype(np.float16)
    V = rng.standard_normal((heads, L, 64)).astype(np.float16)
    dO = rng.standard_normal((heads, M, 64)).astype(np.float16)
    out = {"K": K, "V": V, "dO": dO}
    if unscaled_q:
        out["q"] = (Qs / (LOG2E * 0.125)).astype(np.float16)
        out["Qs"] = qs_as_loaded(out["q"])
    else:
        out["Qs"] = Qs.astype(np.float16)
    return out


def check_property(case, S):
    """Raise AssertionError unless the realised scores S (heads, M, L) have the property the case is named for."""
    M, L = S.shape[-2:]
    nu = L // UNIT
    row = np.arange(M) % 64
    first, rel = lazy_schedule(S)
    if case in ("cold_first_unit", "cold_first_tile"):
        ncold = UNIT if case == "cold_first_unit" else 2 * UNIT
        assert S[..., :ncold].max() <= -150.0 and first.max() <= -140.0 and np.abs(S[..., ncold:]).max() <= 2.0
    elif case == "cold_one_query_block":
        cold = row >= 32
        assert cold.any() and S[:, cold, :UNIT].max() <= -150.0 and first[:, cold].max() <= -140.0
        assert np.abs(S[:, ~cold]).max() <= 5.0 and np.abs(S[..., UNIT:]).max() <= 2.0
    elif case == "late_dominator":
        assert (S[..., -1] - S[..., :-1].max(axis=-1)).min() >= 200.0
    elif case == "stairs_below_threshold":
        assert nu >= 2 and 5.0 <= rel[..., 1:].min() and rel[..., 1:].max() < THR - 0.25        # no unit of any row rescales
    elif case == "stairs_above_threshold":
        assert nu >= 2 and THR + 0.25 < rel[..., 1:].min() and rel[..., 1:].max() <= 7.0        # every unit of every row rescales
    elif case == "one_hot_lane":
        hot, units = row == HOT_ROW, [1] + ([nu - 1] if nu > 2 else [])
        assert hot.any() and (np.bincount(np.arange(M)[hot] // 32, minlength=1) <= 1).all()    # at most one per block of 32 queries
        for u in units:
            assert rel[:, hot, u].min() >= THR + 50.0 - 3.0 and rel[:, ~hot, u].max() < 0.0
        other = np.setdiff1d(np.arange(1, nu), units)
        assert rel[..., other].max(initial=-np.inf) < THR
    elif case == "uniform":
        assert (S.max(axis=-1) - S.min(axis=-1)).max() <= 1e-12
    elif case == "high_plateau":
        assert 900.0 <= S.min() and S.max() <= 1000.0
    elif case == "wide_spread":
        assert -300.0 <= S.min() <= -250.0 and 250.0 <= S.max() <= 300.0
        assert (np.histogram(S, bins=6, range=(-300.0, 300.0))[0] >= S.size // 20).all()       # every sixth of the range is populated
    else:
        raise ValueError(case)
