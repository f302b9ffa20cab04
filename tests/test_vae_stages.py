"""Every stored stage of a ShapeVAE transformer layer (foho_vae_fwd / foho_vae_bwd, csrc/foho_vae.inc, on the GEMM epilogues and attention
kernels of csrc/foho_geo.hip) against the float64 referee of tests/vae_ref64.py, TEACHER-FORCED: `foho_vae_fwd` with `saved` keeps every
intermediate of a layer and the workspace still holds every intermediate of a one-layer backward, so each launch is compared with the
referee's evaluation of THAT launch on the fp16 operands the launch itself read.  Errors do not accumulate across stages, the bounds are
componentwise and derived next to each assertion, and a failure names its stage.  tests/test_vae_transformer.py compares whole stacks with
the float32 module at tolerances this file justifies stage by stage.

Form of every bound:  err <= a 2^-24 B + k 2^-11 |ref| + 2^-24,  B the referee's magnitude bound (the same products with absolute
values), k the fp16 roundings between the stored operands and the stored result, `a` the fp32 work: fixed from a float32-against-float64
evaluation of the same formula on the CPU (`test_float32_emulation_fits_half_of_a`: the emulated worst err / (2^-24 B) over all cases,
doubled for the accumulation order, rounded up), never from a kernel's output.  Token profiles: vae_ref64.CASES.

Which GEMM variant a product gets (gemm() in foho_geo.hip; 256 CUs), by shape (B, L, W, heads, F):
  (1, 128, 128, 2, 128)      every product: GV_128 (K / 64 = 2 < 4), one and two K tiles, one row tile
  (2, 256, 256, 4, 512)      every product: GV_PC (4 to 12 K tiles, tiles <= CUs), two images in one launch, no qk_norm, biases
  (3, 384, 256, 4, 1024)     every product: GV_PC, nine row tiles, three images in one launch, L = 2 x 192
  (8, 256, 1024, 16, 1024)   q | k | v (N = 3072): GV_128, 384 tiles; the N = 1024 products: GV_PC; 8 x 16 x 2 = 256 workgroups: DIRECT backward
  (1, 3072, 1024, 16, 4096)  q | k | v, fc1, dZ (N >= 3072): GV_PHASED192 (192 x 256 tiles); the N = 1024 products: GV_PC
  (2, 1536, 1024, 16, 4096)  the same variants; the image boundary lies on a 192-row tile edge under EP_PACK
  (2, 2048, 1024, 16, 4096)  q | k | v: GV_PHASED (256 x 256 tiles: 2048 % 192 != 0 under EP_PACK); fc1, dZ: GV_PHASED192

Worst err / bound per stage (bound = 1), over the shapes: `cpu` = the float32 emulation (fp32 term only: err / (a 2^-24 B)), `gpu` = an
MI355X, with the case that produced it.
  stage       launch                                   fp32 family   cpu     gpu     case and shape of the gpu figure
  pre         q | k | v projection, EP_PREAFF          fold          0.49    0.989   outlier_channels (3, 384, 256, 4, 1024), second layer of two
  v           the same, V third (not normalised)       fold          0.49    0.990   outlier_channels (3, 384, 256, 4, 1024)
  qk_norm     EP_QKN on the stored pre                 norm          0.43    0.998   gaussian (8, 256, 1024, 16, 1024)
  qs qst kt vt  EP_PACK                                bit for bit
  o           k_geo_attn (bound 3 eps P |V|)                                 0.371   hot_head (8, 256, 1024, 16, 1024)
  nlse        k_geo_attn (bound 8 ulp of fp32)                               0.954   outlier_channels (2, 256, 256, 4, 512)
  x1          projection, EP_RESID | EP_STATS          gemm          0.45    0.999   row_offset (8, 256, 1024, 16, 1024)
  z           fc1, EP_PREAFF (statistics: the merge)   fold          0.49    0.991   gelu_tails (3, 384, 256, 4, 1024)
  h           fc1, EP_GELU                             fold          0.49    0.988   gelu_tails (3, 384, 256, 4, 1024)
  out         fc2, EP_RESID (keep and keep = False)    gemm          0.45    0.997   row_offset (3, 384, 256, 4, 1024)
  dz          EP_GELUBWD                               gemm          0.45    0.972   row_offset (8, 256, 1024, 16, 1024), split form
                 without the underflow term                                  866     tiny_gradient 2^-14 (8, 256, 1024, 16, 1024)
  g1          dy2 GEMM + k_geo_ln_bwd                  gemm, norm    0.45    0.995   large_residual (8, 256, 1024, 16, 1024)
  do          EP_TRANS | EP_DELTA                      gemm          0.45    0.991   outlier_channels (3, 384, 256, 4, 1024), second layer of two
  dot         EP_TRANS                                 bit for bit
  delta       EP_DELTA                                 delta         0.41    0.394   gaussian (2, 1536, 1024, 16, 4096)
  dqkv dQ     k_geo_attn_dq (+ k_vae_qknorm_bwd)       norm          0.43    0.142   tiny_gradient 2^-14 (2, 256, 256, 4, 512)    (0.492 without the underflow term)
  dqkv dK     k_geo_attn_bwd (+ k_vae_qknorm_bwd)      norm          0.43    0.156   tiny_gradient 2^-14 (2, 256, 256, 4, 512)    (0.509)
  dqkv dV     k_geo_attn_bwd                                                 0.491   tiny_gradient 2^-14 (8, 256, 1024, 16, 1024) (0.974)
  dy1         plain GEMM                               gemm          0.45    0.989   outlier_channels (3, 384, 256, 4, 1024), second layer of two
  dx          k_geo_ln_bwd                             norm          0.43    0.998   gelu_tails (3, 384, 256, 4, 1024)

A gpu figure just below 1 is what ONE fp16 rounding gives: half an ulp is 2^-11 of a value just above a power of two, and among 10^5 .. 10^7
outputs some sit there, so wherever the fp32 term is small beside 2^-11 |ref| the worst ratio is the rounding's own 0.97 .. 0.999.  The
figures that say something about the fp32 work are those of the rows where that term IS the bound -- the quiet and the constant rows,
printed as `pre.fp32` and `z.fp32`: 0.054 .. 0.084 and 0.045 .. 0.077 on quiet_rows, 0.014 .. 0.037 and 0.012 .. 0.035 on constant_rows,
i.e. 0.4 .. 3 x 2^-24 B -- and delta's.  No stage exceeded its bound on any case: the tests found no fault in the kernels.  Three referee stages
made wrong on purpose (the - rstd mean s term dropped; bits 1 and 2 swapped in `pos`; GELU's tanh form) made `pre` and `v`, the packed
copies, and `h` fail on the stored data, each alone.
"""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_ref64 as A  # noqa: E402
import test_attention_range as TA  # noqa: E402
import vae_ref64 as R  # noqa: E402

gpu = pytest.mark.gpu

E16 = 2.0 ** -11              # half an ulp of fp16, relative
U32 = 2.0 ** -24              # half an ulp of fp32, relative
FLOOR = 2.0 ** -24            # the smallest fp16 subnormal: results that round to 0
# `a` of each formula family (see the module docstring; the emulated figures are asserted on the CPU below)
A_FOLD = 36.0                 # rstd acc - (rstd mean) s + b': K products in fp32, rsqrt, the row statistics     (emulated 17.6)
A_GEMM = 12.0                 # acc + bias, K <= 4096 products in fp32                                          (emulated 5.4)
A_NORM = 12.0                 # LayerNorm forward / backward over 64 .. 1024 columns: three reductions, rsqrt   (emulated 5.1)
A_DELTA = 4.0                 # a 64-term fp32 dot product                                                      (emulated 1.65)
GELU_ABS = 8e-7               # gelu_erf2's documented absolute error
# gelu_grad = Phi + v phi from A&S 7.1.26: erf to 1.5e-7 + the 1-ulp rcp and exp2 (4 x 2^-24) -> 2e-7 on Phi; v phi inherits exp2's
# argument rounding, v^3 phi(v) / 2 x 2^-23 <= 3e-8 (at v = sqrt 3), and three roundings of a value <= 0.25: 1e-7 together
GELU_GRAD_ABS = 3e-7

#           B, L,   W,    heads, F,    qk_norm
SMALL = [(1, 128, 128, 2, 128, True), (2, 256, 256, 4, 512, False), (3, 384, 256, 4, 1024, True)]
DIRECT = (8, 256, 1024, 16, 1024, True)
LARGE = [(1, 3072, 1024, 16, 4096, True), (2, 1536, 1024, 16, 4096, True)]
LARGE_256 = (2, 2048, 1024, 16, 4096, True)
FWD_CASES = [c for c in R.CASES if c != "tiny_gradient"]          # tiny_gradient's tokens ARE gaussian's
REPEATED = ("quiet_rows", "gelu_tails")
FOHO_VAE_SPLIT_DKV = 1            # include/foho_hip.h


def _params(shapes, cases):
    return [(s, c) for s in shapes for c in cases if s[5] or c not in R.NEEDS_QK_NORM]


FWD_PARAMS = _params(SMALL + [DIRECT], FWD_CASES)
BWD_PARAMS = [(s, c, e) for (s, c) in _params(SMALL + [DIRECT], R.CASES) for e in ((10, 14) if c == "tiny_gradient" else (0,))]
LARGE_PARAMS = _params(LARGE, ("gaussian", "outlier_channels")) + [(LARGE_256, "gaussian")]
ALL_SHAPES = SMALL + [DIRECT] + LARGE + [LARGE_256]


# ---------------------------------------------------------------- layers, packed tensors, records
def _blocks(W, heads, F, layers, qk, seed=0):
    """Layers in the form HipVaeTransformer takes, any hidden size: fused q | k | v rows already [q | k | v][head][d].  Gains and biases of
    every LayerNorm away from (1, 0); weights fp16-representable.  qk False: eps 1e-5 and projection biases (the stand-in's layout)."""
    from followmyhold_amd.vae_transformer import _norm64
    nn = torch.nn
    st = torch.random.get_rng_state()
    torch.manual_seed(100 + seed)
    out = []
    for _ in range(layers):
        eps = 1e-6 if qk else 1e-5
        ln1, ln2 = nn.LayerNorm(W, eps=eps), nn.LayerNorm(W, eps=eps)
        qn, kn = (nn.LayerNorm(64, eps=1e-6), nn.LayerNorm(64, eps=1e-6)) if qk else (None, None)
        mods = dict(ln1=ln1, ln2=ln2, qkv=nn.Linear(W, 3 * W, bias=not qk), proj=nn.Linear(W, W), fc1=nn.Linear(W, F), fc2=nn.Linear(F, W), qn=qn, kn=kn)
        with torch.no_grad():
            for m in mods.values():
                if isinstance(m, nn.LayerNorm):
                    m.weight.add_(0.3 * torch.randn_like(m.weight)), m.bias.add_(0.2 * torch.randn_like(m.bias))
            for m in mods.values():
                for p in (m.parameters() if m is not None else ()):
                    p.copy_(p.half().float())
        out.append(dict(qkv=[(ln1, mods["qkv"], None)], heads=heads, q_norm=_norm64(qn, "q_norm"), k_norm=_norm64(kn, "k_norm"), proj=mods["proj"], ln2=ln2,
                        fc1=mods["fc1"], fc2=mods["fc2"]))
    torch.random.set_rng_state(st)
    return out


def _transformer(shape, device, layers=1):
    from followmyhold_amd.vae_transformer import HipVaeTransformer
    B, L, W, heads, F, qk = shape
    return HipVaeTransformer(_blocks(W, heads, F, layers, qk), device=device)


def _setup(case, shape, device, layers=1, scale_exp=10):
    B, L, W, heads, F, qk = shape
    tr = _transformer(shape, device, layers)
    data = R.build(case, B, L, W, heads, F, scale_exp=scale_exp)
    if data["adjust"] is not None:
        for t in tr.t:
            data["adjust"](t)
    return tr, data


def _eps(tr, i=0):
    return float(tr.layers[i].eps1), float(tr.layers[i].eps2)      # as the kernels get them: rounded to float32


def _r256(n):
    return (n + 255) & ~255


def _record_fields(M, W, F, heads, any_qk):
    """vae_saved() of foho_vae.inc, in its order: (name, bytes, dtype, shape)"""
    h, f = torch.float16, torch.float32
    return [("x", M * W * 2, h, (M, W)), ("qkv", M * 3 * W * 2, h, (M, 3 * W)), ("pre", M * 3 * W * 2 if any_qk else 0, h, (M, 3 * W)),
            ("o", M * W * 2, h, (M, W)), ("nlse", M * heads * 4, f, (M, heads)), ("x1", M * W * 2, h, (M, W)), ("z", M * F * 2, h, (M, F)),
            ("qs", M * W * 2, h, (M, W)), ("qst", W * M * 2, h, (W, M)), ("kt", W * M * 2, h, (W, M))]


def _workspace_fields(lib, B, L, W, F, heads):
    """vae_layout() of foho_vae.inc, in its order"""
    M = B * L
    h, f, u = torch.float16, torch.float32, torch.uint8
    sd = int(lib.foho_sdpa_workspace_bytes(L, L, heads))
    return [("sdpa", sd, u, (sd,)), ("stats", M * (W // 64) * 8, f, (M, W // 64, 2)), ("rowstat", M * 8, f, (M, 2)), ("h", M * F * 2, h, (M, F)),
            ("xa", M * W * 2, h, (M, W)), ("xb", M * W * 2, h, (M, W)), ("qkv", M * 3 * W * 2, h, (M, 3 * W)), ("o", M * W * 2, h, (M, W)),
            ("x1", M * W * 2, h, (M, W)), ("dqkv", M * 3 * W * 2, h, (M, 3 * W)), ("dot", W * M * 2, h, (W, M)), ("vtb", W * M * 2, h, (W, M)),
            ("deltab", M * heads * 4, f, (M, heads))]


def _offsets(fields):
    """running sums of the 256-byte-rounded sizes -> ({name: offset}, total)"""
    off, at = {}, 0
    for name, nbytes, _, _ in fields:
        off[name] = at
        at += _r256(nbytes)
    return off, at


def _views(buf, fields, base=0, only=None):
    """{name: tensor} over the byte buffer `buf`, each a COPY (the buffers are overwritten by the next call)"""
    off, _ = _offsets(fields)
    out = {}
    for name, nbytes, dt, shape in fields:
        if nbytes and (only is None or name in only):
            out[name] = buf[base + off[name]:base + off[name] + nbytes].view(dt).reshape(shape).clone()
    return out


# ---------------------------------------------------------------- ratios
WORST = {}


def _check(tag, stage, got, ref, tol, raw_tol=None):
    """assert |got - ref| <= tol componentwise; print (and keep) the worst err / tol of the stage"""
    got, ref, tol = R.f64(got), R.f64(ref), R.f64(tol)
    bad = ~torch.isfinite(got)
    assert not bad.any(), f"{tag}: {stage} is not finite ({int(bad.sum())} of {got.numel()}) where the referee is"
    assert torch.isfinite(ref).all() and (tol > 0).all()
    err = (got - ref).abs()
    r = float((err / tol).max())
    msg = f"RATIO {stage:10s} {r:8.3f}  {tag}"
    if raw_tol is not None:
        msg += f"  (without the underflow term {float((err / R.f64(raw_tol)).max()):.3f})"
    print(msg)
    WORST[stage] = max(WORST.get(stage, (0.0, "")), (r, tag))
    assert r <= 1.0, f"{tag}: {stage} exceeds its bound by the factor {r:.2f}"
    return r


def _tol(a, B, ref, k=1):
    """a 2^-24 B + k 2^-11 |ref| + 2^-24"""
    return a * U32 * B + k * E16 * ref.abs() + FLOOR


def _tol_resid(val, y, By):
    # fp16(fp16(acc + b) + r): the accumulator and bias in fp32 (a 2^-24 B_y), y rounded to fp16 (2^-11 |y|), the sum of two fp16 values is
    # exact in fp32 and is rounded once more (2^-11 |value|); either rounding may land on a subnormal (2^-24 in all)
    return A_GEMM * U32 * By + E16 * y.abs() + E16 * val.abs() + FLOOR


def _tol_h(z, Bz, h):
    # h = fp16(gelu_erf2(z_fp32)): the GELU is taken of the fp32 pre-activation, not of the stored z.  |gelu'| <= 1.13 carries z's fp32
    # error; gelu_erf2's own absolute error; its last fma `(-|v| / 2) r + max(v, 0)` rounds at |z| (2 x 2^-24 |z|); one fp16 rounding
    return 1.13 * A_FOLD * U32 * Bz + GELU_ABS + 2.0 * U32 * z.abs() + E16 * h.abs() + FLOOR


# ---------------------------------------------------------------- the referee and the cases, without a GPU
def _pack64(p):
    """the packed tensors of a layer in float64, nothing rounded (vae_transformer._fold's algebra)"""
    d = lambda a: a.detach().double()
    ws, bs, ss = [], [], []
    for ln, lin, perm in p["qkv"]:
        Wt = d(lin.weight)
        b = (d(lin.bias) if lin.bias is not None else torch.zeros(Wt.shape[0], dtype=torch.float64)) + Wt @ d(ln.bias)
        wf = Wt * d(ln.weight)[None, :]
        if perm is not None:
            wf, b = wf[perm], b[perm]
        ws.append(wf), bs.append(b), ss.append(wf.sum(dim=1))
    fold = [torch.cat(bs), torch.cat(ss)]
    if p["q_norm"] is not None:
        for g, b, eps in (p["q_norm"], p["k_norm"]):
            fold.append(torch.cat([g.double(), b.double(), torch.tensor([eps, 0.0, 0.0, 0.0], dtype=torch.float64)]))
    Wt = d(p["fc1"].weight)
    w1 = Wt * d(p["ln2"].weight)[None, :]
    t = dict(w_qkv=torch.cat(ws), fold_qkv=torch.cat(fold), w_proj=d(p["proj"].weight), b_proj=d(p["proj"].bias), w_fc1=w1,
             fold_fc1=torch.cat([d(p["fc1"].bias) + Wt @ d(p["ln2"].bias), w1.sum(dim=1)]), w_fc2=d(p["fc2"].weight), b_fc2=d(p["fc2"].bias))
    for n in ("w_qkv", "w_proj", "w_fc1", "w_fc2"):
        t[n + "_t"] = t[n].t().contiguous()
    return t


@pytest.mark.parametrize("layout", ["hy3dgen", "hy3dgen_plain", "standin"])
def test_referee_chain_is_the_float64_module_and_its_autograd(layout):
    from followmyhold_amd import standins
    from followmyhold_amd.vae_transformer import _blocks as module_blocks
    torch.manual_seed(3)
    if layout == "standin":
        vae = standins.StandInShapeVAE(num_latents=128, embed_dim=8, width=128, heads=2, layers=1, num_freqs=4)
    else:
        vae = standins.Hy3dgenLayoutShapeVAE(num_latents=128, embed_dim=8, width=128, heads=2, layers=1, num_freqs=4, qk_norm=layout == "hy3dgen",
                                             qkv_bias=layout == "hy3dgen_plain")
    with torch.no_grad():
        for m in vae.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(0.3 * torch.randn_like(m.weight)), m.bias.add_(0.2 * torch.randn_like(m.bias))
    vae = vae.double().requires_grad_(False)
    p = module_blocks(vae)[0]
    t = _pack64(p)
    qk = p["q_norm"] is not None
    eps1, eps2 = float(p["qkv"][0][0].eps), float(p["ln2"].eps)
    Bn, L = 2, 128
    x = (torch.randn(Bn, L, 128, dtype=torch.float64) + 3.0).requires_grad_(True)
    g = torch.randn(Bn, L, 128, dtype=torch.float64)
    want = vae.block_forward(vae.transformer.resblocks[0], x) if layout != "standin" else vae.transformer[0](x)
    want.backward(g)
    r = R.layer_forward(x.detach().reshape(Bn * L, 128), t, eps1, eps2, 2, Bn, qk)
    assert (r["out"] - want.detach().reshape(Bn * L, 128)).abs().max() <= 1e-10
    b = R.layer_backward(r, g.reshape(Bn * L, 128), t, eps1, eps2, 2, Bn, qk)
    assert (b["dx"] - x.grad.reshape(Bn * L, 128)).abs().max() <= 1e-9
    # the statistics of the two routes: part records merged (EP_STATS + k_geo_rowstat_finish) against the plain row statistics
    for got, want_ in zip(R.merge_stats(R.part_stats(r["x1"]), eps2), R.rowstat(r["x1"], eps2)):
        assert ((got - want_).abs() <= 1e-12 * want_.abs().clamp(min=1.0)).all()


def test_every_stage_value_is_within_its_magnitude_bound():
    shape = SMALL[0]
    B, L, W, heads, F, qk = shape
    tr, data = _setup("row_offset", shape, "cpu")
    t, (eps1, eps2) = tr.t[0], _eps(tr)
    x, g = data["x"].reshape(-1, W), data["g"].reshape(-1, W)
    b1, s1, norms = R.split_fold_qkv(t["fold_qkv"], W, qk)
    within = lambda v, Bd: bool((v.abs() <= Bd * (1 + 1e-12)).all())
    r = R.layer_forward(x, t, eps1, eps2, heads, B, qk)
    assert within(r["pre"], r["B_pre"]) and within(r["y1"], r["B_y1"]) and within(r["z"], r["B_z"]) and within(r["y2"], r["B_y2"])
    assert within(*R.qk_norm(r["pre"][:, :W], *norms[0]))
    bw = R.layer_backward(r, g, t, eps1, eps2, heads, B, qk)
    _, acc, Bacc, _ = R.dz(g, t["w_fc2_t"], r["z"])
    assert within(acc, Bacc) and within(*R.matmul_t(bw["dz"], t["w_fc1_t"]))
    assert within(*R.ln_bwd(r["x1"], bw["dy2"], g, eps2)) and within(*R.do_delta(bw["g1"], t["w_proj_t"], r["o"], heads)[:2])
    assert within(*R.delta_of(bw["do"], r["o"], heads)) and within(*R.qk_norm_bwd(r["pre"][:, W:2 * W], bw["dqkv_attn"][:, W:2 * W], norms[1][0], norms[1][2]))


def test_packed_transpose_is_the_literal_loop():
    a = torch.arange(32 * 64, dtype=torch.float32).reshape(32, 64)
    want = torch.empty(64, 32)
    for m in range(32):
        low = m & 15
        p = (m - low) + (low & 3) + (8 if low & 4 else 0) + (4 if low & 8 else 0)      # bits 2 and 3 of (m & 15) change places
        for c in range(64):
            want[c][p] = a[m][c]
    assert torch.equal(R.packed_transpose(a, 32, False), want)
    both = R.packed_transpose(torch.cat([a, a + 5000.0]), 32, True)
    assert torch.equal(both[0], want) and torch.equal(both[1], want + 5000.0)
    assert [int(R.pos(torch.tensor(m))) for m in (0, 3, 4, 8, 12, 15, 20)] == [0, 3, 8, 4, 12, 15, 24]


def test_merge_of_part_statistics_is_the_row_statistic():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(40, 1024, generator=g, dtype=torch.float64) * 3.0 + 30.0 * torch.randn(40, 1, generator=g, dtype=torch.float64)
    x[:, 70] = 500.0
    x[7] = 2.0
    for eps in (1e-6, 1e-5):
        for got, want in zip(R.merge_stats(R.part_stats(x), eps), R.rowstat(x, eps)):
            assert ((got - want).abs() <= 1e-12 * want.abs().clamp(min=1.0)).all()


@pytest.mark.parametrize("shape,case", _params(SMALL + [DIRECT], R.CASES) + LARGE_PARAMS)
def test_cases_have_the_named_property_at_every_gpu_shape(shape, case):
    """A condition, not a measurement: a case whose rounded operands lose its point fails HERE, without a GPU.  (At the large shapes the two
    cases' properties are properties of the tokens alone: the referee's layer is not run on them here.)"""
    B, L, W, heads, F, qk = shape
    for e in ((10, 14) if case == "tiny_gradient" else (10,)):
        tr, data = _setup(case, shape, "cpu", scale_exp=e)
        assert data["x"].dtype == torch.float16 and data["g"].dtype == torch.float16
        R.check_property(case, data["x"].reshape(-1, W), tr.t[0], *_eps(tr), heads, B, qk, g16=data["g"].reshape(-1, W), layer=L <= 384)


@pytest.mark.parametrize("shape", ALL_SHAPES)
@pytest.mark.parametrize("layers", [1, 2])
def test_record_and_workspace_offsets_add_up_to_the_exported_sizes(shape, layers):
    """A layout change in vae_saved / vae_layout fails here, loudly, instead of making the GPU tests read the wrong bytes."""
    B, L, W, heads, F, qk = shape
    if W * F > 1024 * 1024 and layers == 2:
        layers = 1
    tr = _transformer((1, 128, W, heads, F, qk), "cpu", layers)
    d = tr._desc(B, L)
    M = B * L
    _, per_layer = _offsets(_record_fields(M, W, F, heads, qk))
    assert int(tr.lib.foho_vae_saved_bytes(ctypes.byref(d))) == per_layer * layers
    _, total = _offsets(_workspace_fields(tr.lib, B, L, W, F, heads))
    assert int(tr.lib.foho_vae_workspace_bytes(ctypes.byref(d))) == total


@contextlib.contextmanager
def _referee_in_float32():
    """(one thread: the order of a float32 sum, and so the figure, does not depend on how many cores the machine lends)"""
    n = torch.get_num_threads()
    R.F64 = torch.float32
    torch.set_num_threads(1)
    try:
        yield
    finally:
        R.F64 = torch.float64
        torch.set_num_threads(n)


EMULATED = {}


@pytest.mark.parametrize("shape,case", _params([SMALL[1], SMALL[2]], FWD_CASES) + [(DIRECT, "gaussian"), (DIRECT, "outlier_channels"), (DIRECT, "quiet_rows")])
def test_float32_emulation_fits_half_of_a(shape, case):
    """Where `a` comes from: the referee's own formulas evaluated in float32 (fp32 products and sums, fp32 statistics) against float64, on
    the same fp16 operands -- err / (2^-24 B) per formula family must stay within a / 2 (the other half: the kernels' accumulation order)."""
    B, L, W, heads, F, qk = shape
    tr, data = _setup(case, shape, "cpu")
    t, (eps1, eps2) = tr.t[0], _eps(tr)
    x, g = data["x"].reshape(-1, W), data["g"].reshape(-1, W)
    r = R.layer_forward(x, t, eps1, eps2, heads, B, qk)
    bw = R.layer_backward(r, g, t, eps1, eps2, heads, B, qk)
    b1, s1, norms = R.split_fold_qkv(t["fold_qkv"], W, qk)
    h16 = lambda a: a.half()
    x1, pre16, dz16, g1, do16, o16, dq16 = h16(r["x1"]), h16(r["pre"]), h16(bw["dz"]), h16(bw["g1"]), h16(bw["do"]), h16(r["o"]), h16(bw["dqkv_attn"])
    calls = {
        "fold": [lambda: R.qkv_pre(x, *R.rowstat(x, eps1), t["w_qkv"], b1, s1), lambda: R.fc1_pre(x1, *R.rowstat(x1, eps2), t["w_fc1"], t["fold_fc1"][:F], t["fold_fc1"][F:]),
                 lambda: R.fc1_pre(x1, *R.merge_stats(R.part_stats(x1), eps2), t["w_fc1"], t["fold_fc1"][:F], t["fold_fc1"][F:])],
        "gemm": [lambda: R.proj_resid(o16, t["w_proj"], t["b_proj"], x)[1:], lambda: R.fc2_resid(h16(r["h"]), t["w_fc2"], t["b_fc2"], x1)[1:],
                 lambda: R.matmul_t(dz16, t["w_fc1_t"]), lambda: R.matmul_t(g1, t["w_proj_t"])],
        "norm": [lambda: R.ln_bwd(x1, h16(bw["dy2"]), g, eps2), lambda: R.ln_bwd(x, h16(bw["dy1"]), g1, eps1)] + ([
            lambda: R.qk_norm(pre16[:, :W], *norms[0]), lambda: R.qk_norm(pre16[:, W:2 * W], *norms[1]),
            lambda: R.qk_norm_bwd(pre16[:, :W], dq16[:, :W], norms[0][0], norms[0][2])] if qk else []),
        "delta": [lambda: R.delta_of(do16, o16, heads)],
    }
    limit = {"fold": A_FOLD, "gemm": A_GEMM, "norm": A_NORM, "delta": A_DELTA}
    for fam, fs in calls.items():
        worst = 0.0
        for f in fs:
            ref, Bd = f()
            with _referee_in_float32():
                got = f()[0]
            assert got.dtype == torch.float32 and ref.dtype == torch.float64
            worst = max(worst, float(((got.double() - ref).abs() / (U32 * Bd + 1e-300)).max()))
        EMULATED[(fam, case, shape)] = worst
        print(f"EMULATED {fam:6s} {worst:7.3f}  {case} {shape[:5]}")
    for fam in calls:
        assert EMULATED[(fam, case, shape)] <= limit[fam] / 2.0, (fam, case, EMULATED[(fam, case, shape)])


# ---------------------------------------------------------------- GPU: forward
def _forward_record(tr, x, shape, device, layer=0):
    """one kept forward -> (record of `layer` incl. vt, h and the output where they are that layer's, on `device`; the saved buffer)"""
    B, L, W, heads, F, qk = shape
    M = B * L
    out, saved = tr.forward_raw(x.cuda(), keep=True)
    torch.cuda.synchronize()
    fields = _record_fields(M, W, F, heads, qk)
    rec = _views(saved, fields, base=layer * _offsets(fields)[1])
    if layer == len(tr.layers) - 1:       # the workspace's V^T and h are the last layer's
        ws = _views(tr._workspace(tr._desc(B, L)), _workspace_fields(tr.lib, B, L, W, F, heads), only=("h", "vtb"))
        rec["vt"], rec["h"], rec["out"] = ws["vtb"], ws["h"], out.reshape(M, W).clone()
    return {k: v.to(device) for k, v in rec.items()}, saved


def _assert_projection_stages(tag, rec, x_in, t, shape, eps1, special=None):
    """special: a row mask -- the same assertion once more on those rows alone (quiet / constant rows: where the fp32 term IS the bound)"""
    B, L, W, heads, F, qk = shape
    M = B * L
    assert torch.equal(rec["x"], x_in.reshape(M, W).to(rec["x"].device)), f"{tag}: the saved x is not the input"
    b1, s1, norms = R.split_fold_qkv(t["fold_qkv"], W, qk)
    # pre = fp16(rstd acc - (rstd mean) s + b'): the referee takes (rstd, rstd mean) from the stored x in float64; k_vae_rowstat's fp32
    # two-pass statistics (rsqrt: 1 ulp; the variance to a few 2^-24 relative, second-order in the mean's error) are part of `a`; k = 1
    pre, Bp = R.qkv_pre(rec["x"], *R.rowstat(rec["x"], eps1), t["w_qkv"], b1, s1)
    tol = _tol(A_FOLD, Bp, pre)
    if special is not None:
        _check(tag, "pre.fp32", rec["pre" if qk else "qkv"][special, :2 * W], pre[special, :2 * W], tol[special, :2 * W])
    if qk:
        _check(tag, "pre", rec["pre"][:, :2 * W], pre[:, :2 * W], tol[:, :2 * W])       # (the v third of `pre` is never written nor read)
        _check(tag, "v", rec["qkv"][:, 2 * W:], pre[:, 2 * W:], tol[:, 2 * W:])
        for i, (g, b, eps) in enumerate(norms):
            # q, k = fp16(LayerNorm64(stored fp16 pre) gain + bias): fp32 mean / deviations / rsqrt of 64 values (a 2^-24 B, B with the
            # magnitudes that cancel in x - mean), one fp16 rounding from the STORED pre (two from the accumulator)
            ref, Bn = R.qk_norm(rec["pre"][:, i * W:(i + 1) * W], g, b, eps)
            _check(tag, "qk_norm", rec["qkv"][:, i * W:(i + 1) * W], ref, _tol(A_NORM, Bn, ref))
    else:
        _check(tag, "pre", rec["qkv"][:, :2 * W], pre[:, :2 * W], tol[:, :2 * W])
        _check(tag, "v", rec["qkv"][:, 2 * W:], pre[:, 2 * W:], tol[:, 2 * W:])
    q, k, v = (rec["qkv"][:, i * W:(i + 1) * W] for i in range(3))
    # the packed copies: bit for bit
    assert torch.equal(rec["qs"], R.qs(q)), f"{tag}: qs is not one fp32 product of the stored q with log2(e) / 8, rounded"
    assert torch.equal(rec["qst"], R.packed_transpose(rec["qs"], M, False)), f"{tag}: qst"
    assert torch.equal(rec["kt"].reshape(B, W, L), R.packed_transpose(k, L, True)), f"{tag}: kt"
    if "vt" in rec:
        assert torch.equal(rec["vt"].reshape(B, W, L), R.packed_transpose(v, L, True)), f"{tag}: vt"


def _assert_attention_stage(tag, rec, shape, rows=None):
    """o and nlse against attn_ref64.forward on the stored Qs, K, V, at the bounds of test_attention_range (3 eps P |V| + 2^-24; 8 ulp of
    fp32 at the scores' magnitude).  rows: a sample of the queries (every key, every head) -- the referee's cost is queries x keys."""
    B, L, W, heads, F, qk = shape
    k, v = rec["qkv"][:, W:2 * W], rec["qkv"][:, 2 * W:]
    Qs, O16, K, V = (R.to_heads(a, B, heads) for a in (rec["qs"], rec["o"], k, v))
    nlse = rec["nlse"].reshape(B, L, heads).permute(0, 2, 1).reshape(B * heads, L).double().cpu().numpy()
    if rows is not None:
        Qs, O16, nlse = Qs[:, rows], O16[:, rows], nlse[:, rows]
    for lo in range(0, Qs.shape[0], 4):        # four (image, head) pairs at a time: the score matrices stay small
        sl = slice(lo, lo + 4)
        op = {"Qs": Qs[sl], "K": K[sl], "V": V[sl]}
        op["S"], op["P"], op["O"], op["lse2"] = A.forward(op["Qs"], op["K"], op["V"])
        TA._assert_O(tag, O16[sl], op, op["P"] @ np.abs(op["V"].astype(np.float64)))
        TA._assert_lse(tag, nlse[sl], -nlse[sl] * A.LN2, op, Qs.shape[1])


def _assert_mlp_stages(tag, rec, t, shape, eps2, special=None):
    B, L, W, heads, F, qk = shape
    x1, y1, By1 = R.proj_resid(rec["o"], t["w_proj"], t["b_proj"], rec["x"])
    _check(tag, "x1", rec["x1"], x1, _tol_resid(x1, y1, By1))
    # z = fp16(rstd acc - (rstd mean) s + b') with the statistics of the stored x1 -- which cannot be read back (`stats`, `rowstat` are
    # overwritten by fc2's epilogue): they are checked THROUGH z, the referee taking them from the stored x1 in float64.
    # dz / d mean = -rstd s[n] and dz / d rstd = (z - b') / rstd.  A wrong merge of the part MEANS shows most on quiet_rows and
    # constant_rows: rstd = 350 .. 1000 there against 1 on a Gaussian row, so an error of the merged mean of 2^-20 (relative to a mean of 2)
    # moves z by rstd |s| 2e-6 = 1e-3 .. 1e-2 |s|, where the bound is a 2^-24 rstd (|x1| |Wf|) -- the SAME rstd times what 2^-24 is relative
    # to.  (On constant rows acc - mean s = 0: z = b' whatever rstd is, so only the mean is tested there.)  A wrong merge of the M2 records
    # (the 64 (mean_i - mean)^2 term) shows on outlier_channels, where the parts that hold an outlier have means 1 .. 1.5 away from the
    # row's and that term is most of the variance: rstd moves by its own size and z with it, against 2^-11 |z|.
    z, Bz = R.fc1_pre(rec["x1"], *R.merge_stats(R.part_stats(rec["x1"]), eps2), t["w_fc1"], t["fold_fc1"][:F], t["fold_fc1"][F:])
    _check(tag, "z", rec["z"], z, _tol(A_FOLD, Bz, z))
    if special is not None:
        _check(tag, "z.fp32", rec["z"][special], z[special], _tol(A_FOLD, Bz, z)[special])
    h = R.gelu(z)
    _check(tag, "h", rec["h"], h, _tol_h(z, Bz, h))
    out, y2, By2 = R.fc2_resid(rec["h"], t["w_fc2"], t["b_fc2"], rec["x1"])
    _check(tag, "out", rec["out"], out, _tol_resid(out, y2, By2))
    return out, _tol_resid(out, y2, By2)


@gpu
@pytest.mark.parametrize("shape,case", FWD_PARAMS)
def test_forward_stages(shape, case):
    B, L, W, heads, F, qk = shape
    tr, data = _setup(case, shape, "cuda")
    t = {k: v.cpu() for k, v in tr.t[0].items()}
    eps1, eps2 = _eps(tr)
    tag = f"{case} {shape[:5]}"
    rec, saved = _forward_record(tr, data["x"], shape, "cpu")
    special = (R._rows(B * L, 1) | (R._rows(B * L, 3) & (case == "quiet_rows"))) if case in ("quiet_rows", "constant_rows") else None
    _assert_projection_stages(tag, rec, data["x"], t, shape, eps1, special)
    _assert_attention_stage(tag, rec, shape)
    out, tol = _assert_mlp_stages(tag, rec, t, shape, eps2, special)
    if case in ("constant_rows", "quiet_rows"):        # the projection is zero in these cases: x1 IS x, the rows keep their profile
        assert torch.equal(rec["x1"], rec["x"])
    # keep = False (the inference route: other epilogue instantiations, nothing saved): the same bound as the kept output
    plain = tr.forward_raw(data["x"].cuda(), keep=False)[0]
    torch.cuda.synchronize()
    _check(tag, "out_plain", plain.reshape(B * L, W).cpu(), out, tol)
    if case in REPEATED:
        rec2, _ = _forward_record(tr, data["x"], shape, "cpu")
        for name, a in rec.items():        # (the v third of `pre` is never written: compared up to it)
            n = 2 * W if name == "pre" else a.shape[1]
            assert torch.equal(rec2[name][:, :n], a[:, :n]), f"{tag}: {name} of a second run differs"


@gpu
@pytest.mark.parametrize("group", ["projection", "attention", "mlp"])
@pytest.mark.parametrize("shape,case", LARGE_PARAMS)
def test_large_forward_stages(shape, case, group):
    """The 192-row and 256-row tiles (M >= 2048 and >= 128 tiles of 256 x 256: nothing smaller reaches them); the referee's matmuls run in
    float64 on the GPU, the attention's on a seventh of the queries (7 is coprime to every tile size: every lane position, every head, every key)."""
    B, L, W, heads, F, qk = shape
    tr, data = _setup(case, shape, "cuda")
    tag = f"{case} {shape[:5]}"
    rec, _ = _forward_record(tr, data["x"], shape, "cuda")
    if group == "projection":
        _assert_projection_stages(tag, rec, data["x"], tr.t[0], shape, _eps(tr)[0])
    elif group == "attention":
        _assert_attention_stage(tag, rec, shape, rows=np.arange(0, L, 7))
    else:
        _assert_mlp_stages(tag, rec, tr.t[0], shape, _eps(tr)[1])


# ---------------------------------------------------------------- GPU: backward
def _tol_dz(acc, Bacc, gp, val, underflow=True):
    # dZ = fp16(fp16(acc) gelu_grad(z16)): the accumulator in fp32, rounded to fp16 (2^-11 |acc|; below 2^-14 the rounding is absolute,
    # 2^-25 whatever the value: the UNDERFLOW term, which a relative bound does not contain), times gelu' (its own absolute error on
    # |acc|), rounded once more (2^-24: the floor of every bound, an underflow term itself)
    inner = A_GEMM * U32 * Bacc + E16 * acc.abs() + (2.0 ** -25 if underflow else 0.0)
    return inner * gp.abs() + GELU_GRAD_ABS * acc.abs() + E16 * val.abs() + (FLOOR if underflow else 2.0 ** -40)


def _attn_grad_refs(rec, dO16, shape, rows=None):
    """the attention backward's referee on the stored operands -> {name: (ref, tol, raw tol)} as (M, W) float64 tensors (CPU), tol the bound of
    test_attention_range._assert_grads: 8 eps B + 2^-24 max |g| + the underflow term (raw: without it).  rows: dQ alone, of those queries
    (dQ of a query needs that query and every key; dK and dV need every query)."""
    B, L, W, heads, F, qk = shape
    k, v = rec["qkv"][:, W:2 * W], rec["qkv"][:, 2 * W:]
    names = ("dQ", "dK", "dV") if rows is None else ("dQ",)
    parts = {n: ([], [], []) for n in names}
    Qs, K, V, dO, O16 = (R.to_heads(a, B, heads) for a in (rec["qs"], k, v, dO16, rec["o"]))
    if rows is not None:
        Qs, dO, O16 = Qs[:, rows], dO[:, rows], O16[:, rows]
    for lo in range(0, B * heads, 4):
        sl = slice(lo, lo + 4)
        op = {"Qs": Qs[sl], "K": K[sl], "V": V[sl], "dO": dO[sl]}
        got = TA._grad_refs_and_bounds(op, O16[sl])
        for n in names:
            ref, Bg, floor, U = got[n]
            for dst, a in zip(parts[n], (ref, 8.0 * TA.EPS * Bg + floor + U, 8.0 * TA.EPS * Bg + floor)):
                dst.append(np.broadcast_to(a, ref.shape))
    return {n: tuple(R.from_heads(np.concatenate(p), B, heads) for p in parts[n]) for n in names}


def _backward_views(tr, g, saved, shape, device):
    """one backward -> every intermediate the workspace still holds, and dX, on `device`"""
    B, L, W, heads, F, qk = shape
    dX = tr.backward_raw(g.cuda(), saved, (B, L, W))
    torch.cuda.synchronize()
    names = {"h": "dz", "xa": "g1", "xb": "xb", "o": "dy1", "x1": "do", "dqkv": "dqkv", "dot": "dot", "deltab": "delta"}
    ws = _views(tr._workspace(tr._desc(B, L)), _workspace_fields(tr.lib, B, L, W, F, heads))
    bw = {names[k]: v.to(device) for k, v in ws.items() if k in names}
    bw["dx"] = dX.reshape(B * L, W).to(device)
    return bw


def _assert_backward_stages(tag, bw, g, rec, t, eps1, eps2, shape, rows=None):
    """Every backward intermediate of ONE layer against its referee stage on the stored operands: g the fp16 gradient the layer was given,
    rec its forward record, bw what the workspace holds after it.  rows: the attention backward on a sample (dQ of those queries only)."""
    B, L, W, heads, F, qk = shape
    M = B * L
    dev = bw["dz"].device
    g = g.reshape(M, W).to(dev)
    val, acc, Bacc, gp = R.dz(g, t["w_fc2_t"], rec["z"])
    _check(tag, "dz", bw["dz"], val, _tol_dz(acc, Bacc, gp, val), raw_tol=_tol_dz(acc, Bacc, gp, val, underflow=False))
    # g1 = fp16(g + LayerNorm'(x1; dy2)), dy2 = fp16(dZ . W_fc1f) is overwritten later: its own bound (k = 1, on the STORED dZ) is carried
    # through the launch by |d LayerNorm^T| (ln_bwd_bound) and k_geo_ln_bwd's own fp32 work and rounding are added
    dy2, B2 = R.matmul_t(bw["dz"], t["w_fc1_t"])
    g1, Bg1 = R.ln_bwd(rec["x1"], dy2, g, eps2)
    _check(tag, "g1", bw["g1"], g1, R.ln_bwd_bound(rec["x1"], _tol(A_GEMM, B2, dy2), eps2) + _tol(A_NORM, Bg1, g1))
    dO, BdO = R.matmul_t(bw["g1"], t["w_proj_t"])
    _check(tag, "do", bw["do"], dO, _tol(A_GEMM, BdO, dO))
    assert torch.equal(bw["dot"], R.packed_transpose(bw["do"], M, False)), f"{tag}: dO^T is not the packed transpose of dO"
    # delta = - sum over a head of (stored dO) x (stored O), 64 fmas and three adds in fp32: no fp16 rounding
    dl, Bdl = R.delta_of(bw["do"], rec["o"], heads)
    _check(tag, "delta", bw["delta"], dl, A_DELTA * U32 * Bdl + 2.0 ** -126)
    ag = _attn_grad_refs(rec, bw["do"], shape, rows)
    _, _, norms = R.split_fold_qkv(t["fold_qkv"], W, qk)
    at = slice(None) if rows is None else (torch.arange(B)[:, None] * L + torch.as_tensor(rows)[None, :]).reshape(-1).to(dev)
    for i, n in enumerate(("dQ", "dK", "dV")):
        if n not in ag:
            continue
        sl = slice(i * W, (i + 1) * W)
        ref, tol, raw = (a.to(dev) for a in ag[n])
        got = bw["dqkv"][at, sl]
        if qk and i < 2:
            # dQ, dK go through k_vae_qknorm_bwd in place: the attention's bound carried through |d qk_norm^T|, plus that kernel's own
            gn, _, eps = norms[i]
            pre = rec["pre"][at, sl]
            via, Bn = R.qk_norm_bwd(pre, ref, gn, eps)
            own = _tol(A_NORM, Bn, via)
            _check(tag, "dqkv_" + n, got, via, R.qk_norm_bwd_bound(pre, tol, gn, eps) + own, raw_tol=R.qk_norm_bwd_bound(pre, raw, gn, eps) + own)
        else:
            _check(tag, "dqkv_" + n, got, ref, tol, raw_tol=raw)
    dy1, B1 = R.matmul_t(bw["dqkv"], t["w_qkv_t"])
    _check(tag, "dy1", bw["dy1"], dy1, _tol(A_GEMM, B1, dy1))
    dx, Bdx = R.ln_bwd(rec["x"], bw["dy1"], bw["g1"], eps1)
    _check(tag, "dx", bw["dx"], dx, _tol(A_NORM, Bdx, dx))


@gpu
@pytest.mark.parametrize("shape,case,scale_exp", BWD_PARAMS)
def test_backward_stages(shape, case, scale_exp):
    B, L, W, heads, F, qk = shape
    tr, data = _setup(case, shape, "cuda", scale_exp=scale_exp or 10)
    t = {k: v.cpu() for k, v in tr.t[0].items()}
    tag = f"{case}{'/2^-%d' % scale_exp if scale_exp else ''} {shape[:5]}"
    rec, saved = _forward_record(tr, data["x"], shape, "cpu")
    direct = B * heads * (L // 128) >= 256          # foho_vae_bwd's own rule
    bw = _backward_views(tr, data["g"], saved, shape, "cpu")
    _assert_backward_stages(tag + (" direct" if direct else " split"), bw, data["g"], rec, t, *_eps(tr), shape)
    if direct:                                      # the same shape through the split form
        tr.flags = FOHO_VAE_SPLIT_DKV
        bw2 = _backward_views(tr, data["g"], saved, shape, "cpu")
        _assert_backward_stages(tag + " split (flag)", bw2, data["g"], rec, t, *_eps(tr), shape)
        assert torch.equal(bw2["do"], bw["do"]) and torch.equal(bw2["delta"], bw["delta"]) and torch.equal(bw2["dz"], bw["dz"])
        tr.flags = 0
    if case in REPEATED:
        again = _backward_views(tr, data["g"], saved, shape, "cpu")
        assert all(torch.equal(again[k], bw[k]) for k in bw if k != "xb"), f"{tag}: a second backward differs"


@gpu
@pytest.mark.parametrize("shape,case", LARGE_PARAMS)
def test_large_backward_stages(shape, case):
    """The backward's GEMMs and row kernels on the large tiles, every stage; of the attention backward dQ on a seventh of the queries (the
    float64 dK and dV of 3072 tokens x 16 heads cost the CPU a minute: they are checked at the small shapes, both forms)."""
    B, L, W, heads, F, qk = shape
    tr, data = _setup(case, shape, "cuda")
    rec, saved = _forward_record(tr, data["x"], shape, "cuda")
    bw = _backward_views(tr, data["g"], saved, shape, "cuda")
    _assert_backward_stages(f"{case} {shape[:5]}", bw, data["g"], rec, tr.t[0], *_eps(tr), shape, rows=np.arange(0, L, 7))


@gpu
@pytest.mark.parametrize("shape,case", [(SMALL[1], "row_offset"), (SMALL[2], "outlier_channels")])
def test_two_layer_backward(shape, case):
    """A two-layer stack.  The second layer's backward intermediates are overwritten by the first's, but its result -- the gradient handed
    to the first layer -- stays in the workspace (`xb`): (1) it equals, bit for bit, a ONE-layer backward of the second layer's weights on
    the second layer's part of the record, whose every stage is asserted; (2) every stage of the first layer's backward, dX included, is
    asserted on its own stored operands with that hand-over as its g.  Together: dX of the stack against the referee chained over both
    layers, each fed its layer's stored record, with no bound looser than the one-layer ones."""
    from followmyhold_amd.vae_transformer import HipVaeTransformer
    B, L, W, heads, F, qk = shape
    blocks = _blocks(W, heads, F, 2, qk, seed=1)
    tr = HipVaeTransformer(blocks, device="cuda")
    data = R.build(case, B, L, W, heads, F)
    ts = [{k: v.cpu() for k, v in t.items()} for t in tr.t]
    rec1, saved = _forward_record(tr, data["x"], shape, "cpu", layer=1)
    fields = _record_fields(B * L, W, F, heads, qk)
    per_layer = _offsets(fields)[1]
    assert saved.numel() == 2 * per_layer
    rec0 = {k: v.cpu() for k, v in _views(saved, fields).items()}
    assert torch.equal(rec0["x"], data["x"].reshape(B * L, W))
    bw = _backward_views(tr, data["g"], saved, shape, "cpu")
    tag = f"two layers {case} {shape[:5]}"
    _assert_backward_stages(tag + " layer 0", bw, bw["xb"], rec0, ts[0], *_eps(tr, 0), shape)
    one = HipVaeTransformer(blocks[1:], device="cuda")
    assert all(torch.equal(one.t[0][k], tr.t[1][k]) for k in one.t[0])
    bw1 = _backward_views(one, data["g"], saved[per_layer:].clone(), shape, "cpu")
    assert torch.equal(bw1["dx"], bw["xb"]), f"{tag}: the gradient handed from layer 1 to layer 0 is not layer 1's one-layer backward"
    _assert_backward_stages(tag + " layer 1", bw1, data["g"], rec1, ts[1], *_eps(tr, 1), shape)
    # the second layer's forward stages on ITS stored operands (its statistics came from fc2's epilogue of the first layer, not k_vae_rowstat)
    _assert_projection_stages(tag + " layer 1", rec1, rec1["x"], ts[1], shape, _eps(tr, 1)[0])
    _assert_mlp_stages(tag + " layer 1", rec1, ts[1], shape, _eps(tr, 1)[1])
