"""A float64 referee for one ShapeVAE transformer layer (foho_vae_fwd / foho_vae_bwd, csrc/foho_vae.inc), one function per launch.

Plain torch in float64, on whatever device its operands are on; nothing of the package is imported.  Every function takes the operands
the launch itself reads -- the packed tensors of `HipVaeTransformer.t[i]` and fp16 activations as the kernels stored them -- and returns
the float64 result together with B, the same expression evaluated with absolute values: the componentwise magnitude every fp32 rounding
on the kernel's path is relative to (as `attn_ref64.bounds` does for the attention, which is reused here, not restated).

Layouts: activations are (M, columns), M = images x tokens, rows of one image contiguous; q | k | v is (M, 3 W) = [Q of all heads | K | V].

The second half builds the token profiles of tests/test_vae_stages.py (`CASES`, `build`) and states, per profile, the property of the
fp16-rounded operands that the profile is named for (`check_property`)."""
import math

import numpy as np
import torch

import attn_ref64 as A

F64 = torch.float64


def f64(t):
    return t.to(F64)


# ---------------------------------------------------------------- forward stages
def rowstat(x, eps):
    """-> (rstd, rstd * mean) of every row: what EP_PREAFF takes (k_vae_rowstat; k_geo_rowstat_finish for the later stages)."""
    x = f64(x)
    mean = x.mean(dim=-1)
    var = (x - mean[:, None]).square().mean(dim=-1)
    rstd = (var + eps).rsqrt()
    return rstd, rstd * mean


def folded_pre(x, rstd, rstd_mean, w, b, s):
    """LayerNorm -> Linear on the un-normalised rows: rstd (x . Wf^T) - (rstd mean) s + b'.  B: the three terms' magnitudes, added."""
    x, w, b, s = f64(x), f64(w), f64(b), f64(s)
    val = rstd[:, None] * (x @ w.t()) - rstd_mean[:, None] * s[None, :] + b[None, :]
    B = rstd.abs()[:, None] * (x.abs() @ w.abs().t()) + rstd_mean.abs()[:, None] * s.abs()[None, :] + b.abs()[None, :]
    return val, B


qkv_pre = folded_pre        # (x, rstd, rstd_mean, w_qkv, b', s): the un-normalised q | k | v projection
fc1_pre = folded_pre        # (x1, rstd, rstd_mean, w_fc1, b', s): the MLP's pre-activation z


def _head_stats(pre, eps):
    """per row and group of 64 columns -> x (M, n, 64), mean, rstd (M, n, 1)"""
    x = f64(pre).reshape(pre.shape[0], -1, 64)
    mean = x.mean(dim=-1, keepdim=True)
    rstd = ((x - mean).square().mean(dim=-1, keepdim=True) + eps).rsqrt()
    return x, mean, rstd


def qk_norm(pre, gain, bias, eps):
    """LayerNorm over each head's 64 columns (pre: (M, heads * 64), one third of the projection).  B = rstd (|x| + |mean|) |gain| + |bias|:
    x - mean cancels, and on a near-constant head rstd is up to eps^-1/2."""
    x, mean, rstd = _head_stats(pre, eps)
    g, b = f64(gain), f64(bias)
    val = (x - mean) * rstd * g + b
    B = rstd * (x.abs() + mean.abs()) * g.abs() + b.abs()
    return val.reshape(pre.shape), B.reshape(pre.shape)


def qs(q16):
    """The scaled copy of Q the attention reads: one float32 product with log2(e) / 8, rounded to fp16."""
    return torch.from_numpy(A.qs_as_loaded(q16.detach().cpu().numpy())).to(q16.device)


def pos(m):
    """m with bits 2 and 3 of (m & 15) swapped: where a matrix-instruction operand built from a C-layout accumulator holds index m."""
    return (m & ~15) | (m & 3) | ((m & 4) << 1) | ((m & 8) >> 1)


def packed_transpose(a, row_len, per_image):
    """T[c][pos(m)] = a[m][c].  per_image False: one (C, M) matrix, row_len = M (all images side by side: Qs^T, dO^T); True: one
    (C, row_len) matrix per image of row_len tokens -> (images, C, row_len) (K^T, V^T)."""
    M, C = a.shape
    assert M % row_len == 0 and (per_image or row_len == M)
    p = pos(torch.arange(row_len, device=a.device))
    src = a.reshape(M // row_len, row_len, C)
    T = torch.empty(M // row_len, C, row_len, dtype=a.dtype, device=a.device)
    T[:, :, p] = src.transpose(1, 2)
    return T if per_image else T[0]


def to_heads(a, n_images, heads):
    """(M, heads * 64) torch -> (images * heads, tokens, 64) numpy, the layout of attn_ref64"""
    M = a.shape[0]
    return a.detach().reshape(n_images, M // n_images, heads, 64).permute(0, 2, 1, 3).reshape(n_images * heads, M // n_images, 64).cpu().numpy()


def from_heads(a, n_images, heads):
    """the inverse of `to_heads` -> (M, heads * 64) float64 torch (CPU)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    L = t.shape[1]
    return t.reshape(n_images, heads, L, 64).permute(0, 2, 1, 3).reshape(n_images * L, heads * 64)


def linear_resid(a, w, b, r):
    """r + a . W^T + b  -> (value, y = a . W^T + b, B_y = |a| . |W|^T + |b|): the residual is added to the ROUNDED y in the kernel."""
    a, w, b = f64(a), f64(w), f64(b)
    y = a @ w.t() + b[None, :]
    return f64(r) + y, y, a.abs() @ w.abs().t() + b.abs()[None, :]


proj_resid = linear_resid   # (o16, w_proj, b_proj, x16) -> x1
fc2_resid = linear_resid    # (h16, w_fc2, b_fc2, x1_16) -> the layer's output


def part_stats(x1):
    """(mean, M2 = sum of squared deviations from it) of every row's 64-column parts -> (M, parts, 2): EP_STATS"""
    x = f64(x1).reshape(x1.shape[0], -1, 64)
    mean = x.mean(dim=-1)
    return torch.stack([mean, (x - mean[..., None]).square().sum(dim=-1)], dim=-1)


def merge_stats(stats, eps):
    """Chan's merge of the parts -> (rstd, rstd * mean): k_geo_rowstat_finish"""
    mean_i, m2_i = stats[..., 0], stats[..., 1]
    n = stats.shape[1]
    mean = mean_i.mean(dim=-1)
    var = (m2_i + 64.0 * (mean_i - mean[:, None]).square()).sum(dim=-1) / (64.0 * n)
    rstd = (var + eps).rsqrt()
    return rstd, rstd * mean


def gelu(z):
    """erf form, 0.5 z erfc(-z / sqrt 2): no cancellation in the negative tail"""
    z = f64(z)
    return 0.5 * z * torch.special.erfc(-z * math.sqrt(0.5))


def gelu_grad(z):
    z = f64(z)
    return 0.5 * torch.special.erfc(-z * math.sqrt(0.5)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


# ---------------------------------------------------------------- backward stages (the weights are constants: dX only)
def matmul_t(a, wt):
    """a . Wt^T -> (value, B): the two plain GEMMs (dy2 = dZ . w_fc1_t^T, dy1 = dQKV . w_qkv_t^T) and every product below"""
    a, wt = f64(a), f64(wt)
    return a @ wt.t(), a.abs() @ wt.abs().t()


def dz(g16, w_fc2_t, z16):
    """(g . W_fc2) gelu'(z) -> (value, acc, B_acc, gelu'(z)): the kernel rounds acc to fp16 before the product (EP_GELUBWD)"""
    acc, B = matmul_t(g16, w_fc2_t)
    gp = gelu_grad(z16)
    return acc * gp, acc, B, gp


def _ln_terms(x, eps):
    x = f64(x)
    mean = x.mean(dim=-1, keepdim=True)
    rstd = ((x - mean).square().mean(dim=-1, keepdim=True) + eps).rsqrt()
    return (x - mean) * rstd, rstd * (x.abs() + mean.abs()), rstd          # xhat, its magnitude bound, rstd


def ln_bwd_bound(x16, mag, eps):
    """|d LayerNorm(x)^T| applied to the non-negative `mag`: rstd (mag + mean(mag) + B_xhat mean(mag B_xhat)).  With mag = |d xhat| it is
    the magnitude bound of ln_bwd's second term; with mag = a tolerance on d xhat it is that tolerance carried through the launch."""
    _, bx, rstd = _ln_terms(x16, eps)
    mag = f64(mag)
    return rstd * (mag + mag.mean(dim=-1, keepdim=True) + bx * (mag * bx).mean(dim=-1, keepdim=True))


def ln_bwd(x16, dxhat16, g16, eps):
    """g + LayerNorm'(x; d xhat), gamma = 1 (the gains sit in the folded weights): k_geo_ln_bwd<0> -> (value, B)"""
    xhat, _, rstd = _ln_terms(x16, eps)
    d = f64(dxhat16)
    dx = rstd * (d - d.mean(dim=-1, keepdim=True) - xhat * (d * xhat).mean(dim=-1, keepdim=True))
    return f64(g16) + dx, f64(g16).abs() + ln_bwd_bound(x16, d.abs(), eps)


def do_delta(g1_16, w_proj_t, o16, heads):
    """dO = g1 . W_proj and delta = - sum over each head of dO O (of the UNROUNDED dO: `delta_of` is the stored operands' version)"""
    dO, B = matmul_t(g1_16, w_proj_t)
    return dO, B, -(dO * f64(o16)).reshape(dO.shape[0], heads, 64).sum(dim=-1)


def delta_of(dO16, o16, heads):
    """- sum over each head of dO O, from the values the epilogue multiplies (EP_DELTA) -> (value, B)"""
    p = (f64(dO16) * f64(o16)).reshape(dO16.shape[0], heads, 64)
    return -p.sum(dim=-1), p.abs().sum(dim=-1)


def qk_norm_bwd_bound(pre16, mag, gain, eps):
    """|d qk_norm^T| applied to the non-negative `mag` (one third, (M, heads * 64)): as `ln_bwd_bound`, per head of 64 columns"""
    x, mean, rstd = _head_stats(pre16, eps)
    bx = rstd * (x.abs() + mean.abs())
    m = f64(mag).reshape(x.shape) * f64(gain).abs()
    return (rstd * (m + m.mean(dim=-1, keepdim=True) + bx * (m * bx).mean(dim=-1, keepdim=True))).reshape(pre16.shape)


def qk_norm_bwd(pre16, d16, gain, eps):
    """the backward of `qk_norm` for one third: k_vae_qknorm_bwd -> (value, B)"""
    x, mean, rstd = _head_stats(pre16, eps)
    xhat = (x - mean) * rstd
    dy = f64(d16).reshape(x.shape) * f64(gain)
    dx = rstd * (dy - dy.mean(dim=-1, keepdim=True) - xhat * (dy * xhat).mean(dim=-1, keepdim=True))
    return dx.reshape(pre16.shape), qk_norm_bwd_bound(pre16, f64(d16).abs(), gain, eps)


# ---------------------------------------------------------------- one layer, every stage unrounded (what the float64 module computes)
def split_fold_qkv(fold_qkv, W, qk):
    """fold_qkv = [b' (3 W) | s (3 W) | q_norm 132 | k_norm 132] -> b', s, [(gain, bias, eps)] for q and k (or None)"""
    b, s = fold_qkv[:3 * W], fold_qkv[3 * W:6 * W]
    if not qk:
        return b, s, None
    n = fold_qkv[6 * W:]
    return b, s, [(n[132 * i:132 * i + 64], n[132 * i + 64:132 * i + 128], float(n[132 * i + 128])) for i in range(2)]


def layer_forward(x, t, eps1, eps2, heads, n_images, qk):
    """Every stage of one layer on (M, W) tokens, nothing rounded -> dict of float64 tensors (CPU)."""
    W = x.shape[1]
    F = t["w_fc1"].shape[0]
    b1, s1, norms = split_fold_qkv(t["fold_qkv"], W, qk)
    r = {"x": f64(x)}
    rstd, rm = rowstat(x, eps1)
    r["pre"], r["B_pre"] = qkv_pre(x, rstd, rm, t["w_qkv"], b1, s1)
    r["qkv"] = r["pre"].clone()
    if qk:
        for i, (g, b, eps) in enumerate(norms):
            r["qkv"][:, i * W:(i + 1) * W] = qk_norm(r["pre"][:, i * W:(i + 1) * W], g, b, eps)[0]
    q, k, v = (r["qkv"][:, i * W:(i + 1) * W] for i in range(3))
    r["qs"] = q * (A.LOG2E / 8.0)
    S, P, O, lse2 = A.forward(*(to_heads(a, n_images, heads) for a in (r["qs"], k, v)))
    r["o"], r["lse2"] = from_heads(O, n_images, heads), lse2
    r["x1"], r["y1"], r["B_y1"] = proj_resid(r["o"], t["w_proj"], t["b_proj"], x)
    r["stat2"] = merge_stats(part_stats(r["x1"]), eps2)
    r["z"], r["B_z"] = fc1_pre(r["x1"], *r["stat2"], t["w_fc1"], t["fold_fc1"][:F], t["fold_fc1"][F:])
    r["h"] = gelu(r["z"])
    r["out"], r["y2"], r["B_y2"] = fc2_resid(r["h"], t["w_fc2"], t["b_fc2"], r["x1"])
    return r


def layer_backward(r, g, t, eps1, eps2, heads, n_images, qk):
    """The backward of `layer_forward` from its record r (or a record of STORED values with the same keys) -> dict; dX is r["dx"]."""
    W = r["x"].shape[1]
    _, _, norms = split_fold_qkv(t["fold_qkv"], W, qk)
    b = {}
    b["dz"] = dz(g, t["w_fc2_t"], r["z"])[0]
    b["dy2"] = matmul_t(b["dz"], t["w_fc1_t"])[0]
    b["g1"] = ln_bwd(r["x1"], b["dy2"], g, eps2)[0]
    b["do"], _, b["delta"] = do_delta(b["g1"], t["w_proj_t"], r["o"], heads)
    qkv = f64(r["qkv"])
    h = lambda a: to_heads(a, n_images, heads)
    qs_ = f64(r["qs"]) if "qs" in r else qkv[:, :W] * (A.LOG2E / 8.0)
    dQ, dK, dV, _ = A.backward(h(qs_), h(qkv[:, W:2 * W]), h(qkv[:, 2 * W:]), h(b["do"]), h(f64(r["o"])))
    b["dqkv_attn"] = torch.cat([from_heads(a, n_images, heads) for a in (dQ, dK, dV)], dim=1)
    b["dqkv"] = b["dqkv_attn"].clone()
    if qk:
        for i, (gn, _, eps) in enumerate(norms):
            sl = slice(i * W, (i + 1) * W)
            b["dqkv"][:, sl] = qk_norm_bwd(f64(r["pre"])[:, sl], b["dqkv_attn"][:, sl], gn, eps)[0]
    b["dy1"] = matmul_t(b["dqkv"], t["w_qkv_t"])[0]
    b["dx"] = ln_bwd(r["x"], b["dy1"], b["g1"], eps1)[0]
    return b


# ---------------------------------------------------------------- token profiles
CASES = ("gaussian", "row_offset", "outlier_channels", "quiet_rows", "constant_rows", "large_residual", "gelu_tails", "hot_head", "tiny_gradient")
OUTLIERS = (5, 37, 100)                 # outlier_channels: the three channels (every width here is >= 128)
NEEDS_QK_NORM = ("hot_head",)
HOT_COLUMN = 5                          # hot_head: the dominant column of head 1 of K


def _rows(M, r):
    return torch.arange(M) % 4 == r


def build(case, B, L, W, heads, F, seed=0, scale_exp=10):
    """-> {"x": (B, L, W) fp16 tokens, "g": (B, L, W) fp16 output gradient, "adjust": None or f(t)} on the CPU.  `adjust` changes the packed
    tensors of a layer IN PLACE (their addresses are what the kernels were given) where the case needs other weights or biases.
    tiny_gradient: the gaussian case with g scaled by 2^-scale_exp (10 or 14)."""
    gen = torch.Generator().manual_seed(1000 * CASES.index(case) + seed)
    M = B * L
    x = torch.randn(M, W, generator=gen, dtype=F64)
    g = torch.randn(M, W, generator=gen, dtype=F64)
    adjust = None

    def zero_proj(t):          # x1 = x bit for bit: the rows keep their profile in front of ln_2 / fc1
        t["w_proj"].zero_(), t["w_proj_t"].zero_(), t["b_proj"].zero_()

    if case == "row_offset":
        sign = torch.where(torch.arange(M) % 4 == 0, 1.0, -1.0)
        x = x + torch.where(torch.arange(M) % 2 == 0, 30.0 * sign, 0.0 * sign)[:, None]
    elif case == "outlier_channels":
        for i, c in enumerate(OUTLIERS):
            x[:, c] = (60.0 + 40.0 * torch.rand(M, generator=gen, dtype=F64)) * (1.0 if i % 2 == 0 else -1.0)
    elif case == "quiet_rows":
        k = torch.randint(-2, 3, (M, W), generator=gen).to(F64)
        x = torch.where(_rows(M, 1)[:, None], 2.0 + k * 2.0 ** -9, x)          # an fp16 ulp at 2 is 2^-9, at 100 2^-4
        x = torch.where(_rows(M, 3)[:, None], 100.0 + k * 2.0 ** -4, x)
        adjust = zero_proj
    elif case == "constant_rows":
        c = torch.tensor([0.5, -3.0, 2.0, 17.25], dtype=F64)[(torch.arange(M) // 4) % 4]
        x = torch.where(_rows(M, 1)[:, None], c[:, None].expand(M, W), x)
        adjust = zero_proj
    elif case == "large_residual":
        x = torch.sign(x) * 2.0 ** (11.5 + torch.rand(M, W, generator=gen, dtype=F64))
    elif case == "gelu_tails":
        def adjust(t):
            t["fold_fc1"][:F].copy_(torch.linspace(-12.0, 12.0, F, dtype=F64)[torch.randperm(F, generator=torch.Generator().manual_seed(seed))])
    elif case == "hot_head":
        # head 0 of Q sees channel 0 only, whose normalised value is ~4e-3 on every fourth row: a projection of 1 +- two fp16 ulps;
        # one column of head 1 of K gets a bias of 40
        rows = _rows(M, 2)
        others = x[:, 1:].mean(dim=1)
        x[:, 0] = torch.where(rows, others + 4e-3, x[:, 0])
        wq0 = torch.randn(64, generator=gen, dtype=F64).sign() * (0.3 + 0.4 * torch.rand(64, generator=gen, dtype=F64))

        def adjust(t):
            w, fold = t["w_qkv"], t["fold_qkv"]
            w[:64].zero_()
            w[:64, 0] = wq0.to(w)
            t["w_qkv_t"].copy_(w.t())
            fold[:64] = 1.0
            fold[W + 64 + HOT_COLUMN] = 40.0
            fold[3 * W:6 * W] = w.to(fold.dtype).sum(dim=1)
    elif case == "tiny_gradient":
        gen = torch.Generator().manual_seed(1000 * CASES.index("gaussian") + seed)
        x = torch.randn(M, W, generator=gen, dtype=F64)
        g = torch.randn(M, W, generator=gen, dtype=F64).half().to(F64) * 2.0 ** -scale_exp
    elif case != "gaussian":
        raise ValueError(case)
    return {"x": x.half().reshape(B, L, W), "g": g.half().reshape(B, L, W), "adjust": adjust}


def check_property(case, x16, t, eps1, eps2, heads, n_images, qk, g16=None, layer=True):
    """Raise AssertionError unless the ROUNDED operands (and the referee's unrounded layer on them) have the property the case is named for."""
    M, W = x16.shape
    x = f64(x16)
    assert torch.isfinite(x).all()
    rstd, rm = rowstat(x16, eps1)
    if case == "row_offset":
        off = torch.arange(M) % 2 == 0
        sd = x.std(dim=1)
        assert (x[off].mean(dim=1).abs() / sd[off] >= 25.0).all() and (x[~off].mean(dim=1).abs() / sd[~off] <= 0.5).all()
    elif case == "outlier_channels":
        assert (x[:, list(OUTLIERS)].square().sum(dim=1) / x.square().sum(dim=1) > 0.9).all()
        assert 60.0 <= x[:, list(OUTLIERS)].abs().min() and x[:, list(OUTLIERS)].abs().max() <= 100.0
    elif case == "quiet_rows":
        quiet = _rows(M, 1) | _rows(M, 3)
        assert (rm[quiet].abs() >= 100.0).all() and (rm[~quiet].abs() < 10.0).all()
        for r_, ulp in ((1, 2.0 ** -9), (3, 2.0 ** -4)):
            sd = x[_rows(M, r_)].std(dim=1)
            assert (sd >= 0.5 * ulp).all() and (sd <= 4.0 * ulp).all()
    elif case == "constant_rows":
        rows = _rows(M, 1)
        assert (x[rows].max(dim=1).values == x[rows].min(dim=1).values).all()
        assert torch.allclose(rstd[rows], torch.full_like(rstd[rows], eps1 ** -0.5), rtol=1e-12)
        # the mathematical pre-activation is b': the EXACT row sums of the folded weights cancel the row.  (The packed s is their float32
        # sum: with it the row keeps rstd c (sum w - s), within 2^-24 of the bound's rstd |mean| |s| term.)
        b, s, _ = split_fold_qkv(t["fold_qkv"], W, qk)
        pre = qkv_pre(x16, rstd, rm, t["w_qkv"], b, f64(t["w_qkv"]).sum(dim=1))[0]
        assert (pre[rows] - f64(b)[None, :]).abs().max() <= 1e-9
        packed, Bp = qkv_pre(x16, rstd, rm, t["w_qkv"], b, s)
        assert ((packed[rows] - f64(b)[None, :]).abs() <= 2.0 ** -22 * Bp[rows]).all()
    if case in ("quiet_rows", "constant_rows"):
        assert not t["w_proj"].any() and not t["b_proj"].any()
    if not layer:
        assert case in ("gaussian", "outlier_channels")
        return None
    r = layer_forward(x16, t, eps1, eps2, heads, n_images, qk)
    for name, a in r.items():
        if torch.is_tensor(a):
            assert torch.isfinite(a).all(), name
    if case == "large_residual":
        assert 2.0 ** 11.4 <= x.abs().min() and max(float(a.abs().max()) for a in r.values() if torch.is_tensor(a) and a.dim() == 2) < 65504.0
        upd = (r["out"] - x).abs()
        assert (upd < 2.0).all()                                   # smaller than half an fp16 ulp (4) of every residual value
    elif case == "gelu_tails":
        z = r["z"]
        assert z.min() <= -11.0 and z.max() >= 11.0
        for lo, hi in ((-12.0, -6.0), (-6.0, -3.0), (-3.0, 3.0), (3.0, 12.0)):
            assert ((z > lo) & (z < hi)).double().mean() >= 0.01, (lo, hi)
        h = r["h"]
        assert ((h < 0) & (h.abs() < 2.0 ** -14) & (h.abs() >= 2.0 ** -25)).any()          # a negative fp16 subnormal
    elif case == "hot_head":
        rows = _rows(M, 2)
        pre16 = r["pre"].half()
        _, mean, rs = _head_stats(pre16[:, :64], t["fold_qkv"][6 * W + 128].item())
        assert (rs[rows, 0, 0] * mean[rows, 0, 0].abs() >= 100.0).all()                     # near-constant: a few fp16 ulps around 1
        assert (f64(pre16[rows, :64]).std(dim=1) <= 4.0 * 2.0 ** -10).all()
        kh = f64(pre16[:, W + 64:W + 128])
        assert (kh[:, HOT_COLUMN].square() / kh.square().sum(dim=1) > 0.9).all()
    elif case == "tiny_gradient":
        assert g16 is not None and 0 < f64(g16).abs().max() <= 2.0 ** -7
        b = layer_backward(r, g16, t, eps1, eps2, heads, n_images, qk)
        # the fp16 intermediates underflow: at 2^-10 a share of every one of them is subnormal, at 2^-14 nearly all of it
        share = 0.9 if f64(g16).abs().max() < 2.0 ** -10 else 0.05
        for name in ("dz", "do", "dqkv"):
            assert (b[name].abs() < 2.0 ** -14).double().mean() >= share, name
    return r
