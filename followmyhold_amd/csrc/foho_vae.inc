// foho_vae.inc -- the ShapeVAE transformer of `latent2sdf` (PL:295 `pred = vae(pred)`), forward and backward to its input tokens, on the
// kernels of foho_geo.hip (included at its end, behind geo_host.inc: same translation unit, same GEMM / attention templates, driven through
// geo_host.inc's launchers -- gemm() with an Epi, attn_fwd / attn_bwd / attn_dq / attn_bwd_split with their operand structs).
//
// Reference: third_party_patches/hy3dgen/shapegen/pipelines.py:292-296 (latent2sdf), 1391-1393 / 1507-1509 (the decode under autograd in
// every inner iteration of phases B and C), 1600 (loss.backward()).  hy3dgen's ShapeVAE.forward is post_kl -> Transformer: sixteen
// pre-norm blocks over 3072 tokens of width 1024 (16 heads of 64, MLP 4096, qk_norm).  Per layer and direction that is 77 GFLOP of GEMM
// + 39 (forward) / 97 (backward) GFLOP of attention on M = 3072 rows -- in torch 25 launches per layer and direction (library GEMMs,
// LayerNorm, GELU, residual adds, cat / copy, the attention pair); here 7 per layer forward:
//
//   rowstat(x)                                              (layer 0 only: later layers get it from fc2's epilogue)
//   qkv  = (rstd (x . (W_qkv gamma_1)^T) - rstd mean s + b')  [EP_PREAFF]; per head LayerNorm of q and of k [EP_QKN]   -> (M, 3 W) [Q | K | V]
//          + what the attention kernels stream, written by the same epilogue [EP_PACK]: V^T (forward), scaled Q, Q^T, K^T (kept for the backward)
//   o    = attention(q, k, v)                               k_geo_attn, operands read where the GEMM left them
//   x1   = x + o . W_proj^T + b, row statistics of x1       [EP_RESID | EP_STATS] + k_geo_rowstat_finish
//   h    = gelu(rstd (x1 . (W_fc1 gamma_2)^T) - ...)        [EP_GELU | EP_PREAFF (| EP_SAVEZ: the pre-activation, for the backward)]
//   x'   = x1 + h . W_fc2^T + b, row statistics of x'       [EP_RESID | EP_STATS] + k_geo_rowstat_finish
//
// and 9 backward (weights are constants of the guidance: dX only, no weight gradients):
//
//   dz   = (g . W_fc2) gelu'(z)                             [EP_GELUBWD]
//   dy2  = dz . (W_fc1 gamma_2)        -> g1 = g + LayerNorm'(x1; dy2)       GEMM on the transposed FOLDED weights: d / d xhat comes out
//   do   = g1 . W_proj, do^T, delta = -rowsum(do o) per head                  of the matrix pipe, k_geo_ln_bwd runs with gamma = 1   [EP_TRANS | EP_DELTA]
//   dq, dk, dv = attention'(q, k, v, o, lse; do)            k_geo_attn_bwd (dK, dV), k_geo_attn_dq; k_vae_qknorm_bwd in place
//   dy1  = [dq | dk | dv] . (W_qkv gamma_1)  -> g' = g1 + LayerNorm'(x; dy1)
//
// All images of a batch share the GEMMs (rows = batch x tokens: fuller launches); every attention kernel takes all images in one launch (AttnB).

namespace geo {

// (rstd, rstd * mean) of every row of X (M, width <= 1024) -- what EP_PREAFF takes; one wave per row
__global__ __launch_bounds__(256) void k_vae_rowstat(const h16* __restrict__ X, int M, int width, float eps, float2* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float v[2][8];
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int col = (c * 64 + lane) * 8;
        if (col < width) {
            const half8 h = *reinterpret_cast<const half8*>(X + (size_t)row * width + col);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                v[c][e] = (float)h[e];
                sum += v[c][e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) v[c][e] = 0.0f;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    const float mean = sum / (float)width;
    float sq = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; c++)
        if ((c * 64 + lane) * 8 < width)
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float d = v[c][e] - mean;
                sq += d * d;
            }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
    if (lane == 0) {
        const float rstd = rsqrtf(sq / (float)width + eps);
        out[row] = float2{rstd, rstd * mean};
    }
}

// Backward of qk_norm, in place on the q and k thirds of dQKV (M, 3 W): dx = LayerNorm64'(x = the un-normalised projection; dy), 8 lanes per
// (row, head, q | k), 8 elements each.  norm: q_norm's 132 floats (gain, bias, eps, pad) followed by k_norm's.
__global__ __launch_bounds__(256) void k_vae_qknorm_bwd(h16* __restrict__ dQKV, const h16* __restrict__ PRE, int M, int heads, const float* __restrict__ norm) {
    const int W = heads * 64, ld = 3 * W;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int ch = (int)(i & 7);
    const size_t unit = i >> 3;                     // (row, which, head)
    const int head = (int)(unit % heads), which = (int)((unit / heads) & 1);
    const size_t row = unit / (2 * (size_t)heads);
    if (row >= (size_t)M) return;                   // (whole groups of 8 lanes leave together)
    const float* nrm = norm + 132 * which;
    const size_t at = row * ld + (size_t)which * W + head * 64 + ch * 8;
    const half8 xv = *reinterpret_cast<const half8*>(PRE + at), gv = *reinterpret_cast<const half8*>(dQKV + at);
    float x[8], dy[8], sm = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        x[e] = (float)xv[e];
        sm += x[e];
        dy[e] = (float)gv[e] * nrm[ch * 8 + e];     // d / d xhat
    }
    const float mean = sum8(sm) * (1.0f / 64.0f);
    float sq = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        x[e] -= mean;
        sq += x[e] * x[e];
    }
    const float rstd = rsqrtf(sum8(sq) * (1.0f / 64.0f) + nrm[128]);
    float a = 0.0f, b = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        x[e] *= rstd;                               // xhat
        a += dy[e];
        b += dy[e] * x[e];
    }
    a = sum8(a) * (1.0f / 64.0f), b = sum8(b) * (1.0f / 64.0f);
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = (h16)(rstd * (dy[e] - a - x[e] * b));
    *reinterpret_cast<half8*>(dQKV + at) = o;
}

static int vae_check(const foho_vae_desc* d) {
    if (!d || !d->layers || !d->zeros) return fail(FOHO_ERR_BAD_ARG, "foho_vae: null descriptor / layers / zeros");
    if (d->width <= 0 || d->width % 128 || d->width > 1024) return fail(FOHO_ERR_BAD_ARG, "foho_vae: width must be a multiple of 128, at most 1024");
    if (d->heads <= 0 || d->heads > 16 || d->width != d->heads * 64) return fail(FOHO_ERR_BAD_ARG, "foho_vae: head dimension must be 64");
    if (d->hidden <= 0 || d->hidden % 128) return fail(FOHO_ERR_BAD_ARG, "foho_vae: hidden must be a multiple of 128");
    if (d->n_tokens < 128 || d->n_tokens % 128) return fail(FOHO_ERR_BAD_ARG, "foho_vae: n_tokens must be a multiple of 128");
    if (d->n_layers < 1 || d->batch < 1) return fail(FOHO_ERR_BAD_ARG, "foho_vae: n_layers >= 1, batch >= 1");
    if ((size_t)d->n_tokens * 3 * d->width * 2 >= ((size_t)1 << 31)) return fail(FOHO_ERR_BAD_ARG, "foho_vae: q | k | v of one image exceed 32-bit buffer offsets");
    if ((size_t)d->batch * d->n_tokens >= ((size_t)1 << 30)) return fail(FOHO_ERR_BAD_ARG, "foho_vae: too many rows");
    for (int i = 0; i < d->n_layers; i++) {
        const foho_vae_layer& y = d->layers[i];
        if (!y.w_qkv || !y.fold_qkv || !y.w_proj || !y.b_proj || !y.w_fc1 || !y.fold_fc1 || !y.w_fc2 || !y.b_fc2)
            return fail(FOHO_ERR_BAD_ARG, "foho_vae: null weight pointer");
        if (!(y.eps1 > 0.0f) || !(y.eps2 > 0.0f)) return fail(FOHO_ERR_BAD_ARG, "foho_vae: LayerNorm eps must be positive");
    }
    return FOHO_OK;
}

struct VaeLayout {   // scratch of either direction
    size_t sdpa, stats, rowstat, h, xa, xb, qkv, o, x1, dqkv, dot, vtb, deltab, total;
    SdpaLayout sl;
};
static VaeLayout vae_layout(const foho_vae_desc* d) {
    VaeLayout l{};
    Carve cv;
    const size_t M = (size_t)d->batch * d->n_tokens, W = d->width, F = d->hidden;
    l.sl = sdpa_layout(d->n_tokens, d->n_tokens, d->heads);
    l.sdpa = cv.take(l.sl.total);
    l.stats = cv.take(M * (W / 64) * 8);
    l.rowstat = cv.take(M * 8);
    l.h = cv.take(M * F * 2);
    l.xa = cv.take(M * W * 2);
    l.xb = cv.take(M * W * 2);
    l.qkv = cv.take(M * 3 * W * 2);
    l.o = cv.take(M * W * 2);
    l.x1 = cv.take(M * W * 2);
    l.dqkv = cv.take(M * 3 * W * 2);
    l.dot = cv.take(W * M * 2);        // dO^T of all images (row length M), key-block order of the backward attention's operands
    l.vtb = cv.take(W * M * 2);        // V^T per image, key-permuted: written by the q | k | v projection's epilogue (EP_PACK), read by the forward attention
    l.deltab = cv.take(M * (size_t)d->heads * 4);   // written by the epilogue of the GEMM that produces dO (EP_DELTA)
    l.total = cv.off;
    return l;
}
struct VaeSaved {   // what the forward keeps, per layer (offsets inside a layer's record)
    size_t x, qkv, pre, o, nlse, x1, z, qs, qst, kt, per_layer, total;
};
static VaeSaved vae_saved(const foho_vae_desc* d) {
    VaeSaved l{};
    Carve cv;
    const size_t M = (size_t)d->batch * d->n_tokens, W = d->width, F = d->hidden;
    bool any_qkn = false;
    for (int i = 0; i < d->n_layers; i++) any_qkn |= d->layers[i].qk_norm != 0;
    l.x = cv.take(M * W * 2);
    l.qkv = cv.take(M * 3 * W * 2);
    l.pre = cv.take(any_qkn ? M * 3 * W * 2 : 0);
    l.o = cv.take(M * W * 2);
    l.nlse = cv.take(M * d->heads * 4);
    l.x1 = cv.take(M * W * 2);
    l.z = cv.take(M * F * 2);
    // what the backward attention streams besides q | k | v, written by the projection's epilogue (EP_PACK) instead of three row kernels in
    // the backward: the scaled Q rows, their transpose (row length M: all images side by side) and K^T per image, keys in operand order
    l.qs = cv.take(M * W * 2);
    l.qst = cv.take(W * M * 2);
    l.kt = cv.take(W * M * 2);
    l.per_layer = cv.off;
    l.total = cv.off * d->n_layers;
    return l;
}

// (rstd, rstd mean) of the rows of X (M, width): one wave per row
static void vae_rowstat(hipStream_t s, const h16* X, int M, int width, float eps, float2* rowstat) {
    hipLaunchKernelGGL(k_vae_rowstat, dim3((M + 3) / 4), dim3(256), 0, s, X, M, width, eps, rowstat);
}
// qk_norm's backward in place on dQKV (M, 3 heads x 64), 8 lanes per (row, q | k, head).  PRE: the un-normalised projection; norm: q_norm's 132 floats, then k_norm's
static void vae_qknorm_bwd(hipStream_t s, h16* dQKV, const h16* PRE, int M, int heads, const float* norm) {
    const size_t lanes = (size_t)M * 2 * heads * 8;
    hipLaunchKernelGGL(k_vae_qknorm_bwd, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, dQKV, PRE, M, heads, norm);
}

}  // namespace geo

extern "C" int64_t foho_vae_abi_size(void) { return (int64_t)sizeof(foho_vae_layer) * 1000 + (int64_t)sizeof(foho_vae_desc); }

extern "C" size_t foho_vae_workspace_bytes(const foho_vae_desc* d) {
    if (vae_check(d) != FOHO_OK) return 0;
    return vae_layout(d).total;
}
extern "C" size_t foho_vae_saved_bytes(const foho_vae_desc* d) {
    if (vae_check(d) != FOHO_OK) return 0;
    return vae_saved(d).total;
}

extern "C" int foho_vae_fwd(const foho_vae_desc* d, const void* x0, void* out, void* ws, size_t ws_bytes, void* saved, size_t saved_bytes, void* stream_) {
    if (int rc = vae_check(d)) return rc;
    if (!x0 || !out || !ws) return fail(FOHO_ERR_BAD_ARG, "foho_vae_fwd: null argument");
    const VaeLayout l = vae_layout(d);
    const VaeSaved sv = vae_saved(d);
    if (ws_bytes < l.total) return fail(FOHO_ERR_WORKSPACE, "foho_vae_fwd: workspace too small");
    if (saved && saved_bytes < sv.total) return fail(FOHO_ERR_WORKSPACE, "foho_vae_fwd: `saved` too small");
    hipStream_t s = (hipStream_t)stream_;
    char *base = (char*)ws, *keep = (char*)saved;
    const int B = d->batch, Lt = d->n_tokens, M = B * Lt, W = d->width, F = d->hidden, NH = d->heads, parts = W / 64, n = d->n_layers;
    float* stats = (float*)(base + l.stats);
    float2* rowstat = (float2*)(base + l.rowstat);
    h16* H = (h16*)(base + l.h);
    h16* vtB = (h16*)(base + l.vtb);
    const h16* X = (const h16*)x0;
    if (keep) {   // the first layer's input is part of what the backward reads: kept with the rest (the caller's tensor may be gone by then)
        if (hipMemcpyAsync(keep + sv.x, x0, (size_t)M * W * 2, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(FOHO_ERR_LAUNCH, "foho_vae_fwd: copy failed");
        X = (const h16*)(keep + sv.x);
    }
    vae_rowstat(s, X, M, W, d->layers[0].eps1, rowstat);
    if (!launch_ok("k_vae_rowstat")) return FOHO_ERR_LAUNCH;
    // the attention of all images in ONE launch: 192 workgroups per image do not fill the chip
    AttnFwd at;
    at.ldq = at.ldk = 3 * W, at.Vt = vtB, at.L = Lt, at.ldo = W, at.M = Lt, at.heads = NH, at.qscale = QSCALE, at.images = B;
    at.img.q = at.img.k = (long)Lt * 3 * W, at.img.vt = (long)W * Lt, at.img.o = (long)Lt * W, at.img.nlse = (long)Lt * NH;
    for (int i = 0; i < n; i++) {
        const foho_vae_layer& y = d->layers[i];
        char* rec = keep ? keep + (size_t)i * sv.per_layer : nullptr;
        h16* QKV = (h16*)(rec ? rec + sv.qkv : base + l.qkv);
        h16* PRE = (rec && y.qk_norm) ? (h16*)(rec + sv.pre) : nullptr;
        h16* O = (h16*)(rec ? rec + sv.o : base + l.o);
        float* NLSE = rec ? (float*)(rec + sv.nlse) : nullptr;
        h16* X1 = (h16*)(rec ? rec + sv.x1 : base + l.x1);
        h16* Z = rec ? (h16*)(rec + sv.z) : nullptr;
        const bool last = i == n - 1;
        h16* Xn = last ? (h16*)out : (h16*)(rec ? keep + (size_t)(i + 1) * sv.per_layer + sv.x : base + ((i & 1) ? l.xb : l.xa));
        // q | k | v behind the folded ln_1 (+ qk_norm; + the un-normalised projection when a backward will follow); the epilogue also leaves V^T
        // for the attention below and -- kept -- Qs, Qs^T, K^T for the backward's
        Epi qkv(y.fold_qkv);
        qkv.preaff(rowstat, 3 * W, y.qk_norm != 0);
        qkv.pack(vtB, rec ? (h16*)(rec + sv.qs) : nullptr, rec ? (h16*)(rec + sv.qst) : nullptr, rec ? (h16*)(rec + sv.kt) : nullptr, Lt, M, QSCALE);
        if (PRE) qkv.save_z(PRE, 3 * W);
        if (int rc = gemm(dense(X, y.w_qkv, QKV, M, 3 * W, W), qkv, s)) return rc;
        at.Q = QKV, at.K = QKV + W, at.O = O, at.nlse = NLSE;
        attn_fwd(s, at);
        if (!launch_ok("foho_vae_fwd (attention)")) return FOHO_ERR_LAUNCH;
        if (int rc = gemm(dense(O, y.w_proj, X1, M, W, W), Epi(y.b_proj).resid(X, W).stats(stats, parts), s)) return rc;
        rowstat_finish(s, stats, parts, M, y.eps2, rowstat);
        if (!launch_ok("k_geo_rowstat_finish")) return FOHO_ERR_LAUNCH;
        Epi fc1(y.fold_fc1);
        fc1.gelu().preaff(rowstat, F);
        if (Z) fc1.save_z(Z, F);
        if (int rc = gemm(dense(X1, y.w_fc1, H, M, F, W), fc1, s)) return rc;
        Epi fc2(y.b_fc2);
        fc2.resid(X1, W);
        if (!last) fc2.stats(stats, parts);   // ... of the next layer's input
        if (int rc = gemm(dense(H, y.w_fc2, Xn, M, W, F), fc2, s)) return rc;
        if (!last) {
            rowstat_finish(s, stats, parts, M, d->layers[i + 1].eps1, rowstat);
            if (!launch_ok("k_geo_rowstat_finish")) return FOHO_ERR_LAUNCH;
        }
        X = Xn;
    }
    return FOHO_OK;
}

extern "C" int foho_vae_bwd(const foho_vae_desc* d, const void* grad_out, void* grad_x0, void* ws, size_t ws_bytes, const void* saved, size_t saved_bytes,
                            void* stream_) {
    if (int rc = vae_check(d)) return rc;
    if (!grad_out || !grad_x0 || !ws || !saved) return fail(FOHO_ERR_BAD_ARG, "foho_vae_bwd: null argument");
    const VaeLayout l = vae_layout(d);
    const VaeSaved sv = vae_saved(d);
    if (ws_bytes < l.total) return fail(FOHO_ERR_WORKSPACE, "foho_vae_bwd: workspace too small");
    if (saved_bytes < sv.total) return fail(FOHO_ERR_WORKSPACE, "foho_vae_bwd: `saved` too small");
    for (int i = 0; i < d->n_layers; i++)
        if (!d->layers[i].w_qkv_t || !d->layers[i].w_proj_t || !d->layers[i].w_fc1_t || !d->layers[i].w_fc2_t)
            return fail(FOHO_ERR_BAD_ARG, "foho_vae_bwd: the transposed weights are missing");
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    const char* keep = (const char*)saved;
    const int B = d->batch, Lt = d->n_tokens, M = B * Lt, W = d->width, F = d->hidden, NH = d->heads, n = d->n_layers;
    h16 *H = (h16*)(base + l.h), *G1 = (h16*)(base + l.xa), *GB = (h16*)(base + l.xb), *T1 = (h16*)(base + l.o), *dO = (h16*)(base + l.x1);
    h16 *dQKV = (h16*)(base + l.dqkv), *dOT = (h16*)(base + l.dot);
    float* deltaB = (float*)(base + l.deltab);
    // enough (image, head, key block) workgroups to fill the chip on their own: each writes its dK / dV itself, all images in one launch
    const bool direct = !(d->flags & FOHO_VAE_SPLIT_DKV) && (long)B * NH * (Lt / 128) >= 256;
    const float* nog = nullptr;   // gamma = 1: the gradients come through the folded weights
    const h16* G = (const h16*)grad_out;
    // the attention backward of all images: what does not depend on the layer
    const long i3 = (long)Lt * 3 * W, iw = (long)Lt * W, ih = (long)Lt * NH;
    AttnBwd bk;
    bk.dO = dO, bk.dOT = dOT, bk.ldt = M, bk.ndelta = deltaB, bk.ldkv = 3 * W, bk.width = W, bk.heads = NH, bk.M = Lt, bk.L = Lt, bk.images = B;
    bk.dk16 = dQKV + W, bk.dv16 = dQKV + 2 * W, bk.ld16 = 3 * W;
    bk.img.qs = iw, bk.img.qst = Lt, bk.img.dO = iw, bk.img.dOT = Lt, bk.img.nlse = ih, bk.img.ndelta = ih, bk.img.kv = i3, bk.img.dkv = i3;
    AttnDq dq;
    dq.dO = dO, dq.ldq = W, dq.ldkv = 3 * W, dq.width = W, dq.L = Lt, dq.ndelta = deltaB, dq.dQ = dQKV, dq.lddq = 3 * W, dq.M = Lt, dq.heads = NH, dq.images = B;
    dq.img.qs = iw, dq.img.dO = iw, dq.img.kv = i3, dq.img.kt = (long)W * Lt, dq.img.nlse = ih, dq.img.ndelta = ih, dq.img.dq = i3;
    for (int i = n - 1; i >= 0; i--) {
        const foho_vae_layer& y = d->layers[i];
        const char* rec = keep + (size_t)i * sv.per_layer;
        const h16 *X = (const h16*)(rec + sv.x), *QKV = (const h16*)(rec + sv.qkv), *PRE = (const h16*)(rec + sv.pre), *O = (const h16*)(rec + sv.o);
        const h16 *X1 = (const h16*)(rec + sv.x1), *Z = (const h16*)(rec + sv.z);
        const float* NLSE = (const float*)(rec + sv.nlse);
        const h16 *qsB = (const h16*)(rec + sv.qs), *QsT = (const h16*)(rec + sv.qst), *ktB = (const h16*)(rec + sv.kt);
        h16* Gn = (i == 0) ? (h16*)grad_x0 : GB;
        if (int rc = gemm(dense(G, y.w_fc2_t, H, M, F, W), Epi(d->zeros).gelu_bwd(Z, F), s)) return rc;   // dZ
        if (int rc = gemm(dense(H, y.w_fc1_t, T1, M, W, F), Epi(d->zeros), s)) return rc;                 // d / d xhat of ln_2
        ln_rows_bwd(s, X1, nog, y.eps2, T1, G, G1, M, W);
        if (!launch_ok("k_geo_ln_bwd(2)")) return FOHO_ERR_LAUNCH;
        if (int rc = gemm(dense(G1, y.w_proj_t, dO, M, W, W), Epi(d->zeros).trans(dOT, M).delta(O, W, deltaB, NH), s)) return rc;   // dO, dO^T, delta
        bk.Qs = dq.Qs = qsB, bk.QsT = QsT, dq.Kt = ktB, bk.nlse = dq.nlse = NLSE, bk.KV = dq.KV = QKV + W, bk.Vp = dq.Vp = QKV + 2 * W;
        if (direct) {   // all images in one launch per kernel
            attn_bwd(s, bk);
            attn_dq(s, dq);
            if (!launch_ok("vae attention backward")) return FOHO_ERR_LAUNCH;
        } else {   // (too few (head, key block) workgroups to fill the chip, or FOHO_VAE_SPLIT_DKV): image by image through the stand-alone attention's scratch
            for (int b = 0; b < B; b++)
                if (int rc = attn_bwd_split(s, image_of(bk, b), image_of(dq, b), l.sl.splits, (float*)(base + l.sdpa + l.sl.part))) return rc;
        }
        if (y.qk_norm) {   // (inside the two kernels' way out it cost them 6-9 us each against the 8 us of this launch: NOTEBOOK round 6)
            vae_qknorm_bwd(s, dQKV, PRE, M, NH, y.fold_qkv + 6 * W);
            if (!launch_ok("k_vae_qknorm_bwd")) return FOHO_ERR_LAUNCH;
        }
        if (int rc = gemm(dense(dQKV, y.w_qkv_t, T1, M, W, 3 * W), Epi(d->zeros), s)) return rc;   // d / d xhat of ln_1
        ln_rows_bwd(s, X, nog, y.eps1, T1, G1, Gn, M, W);
        if (!launch_ok("k_geo_ln_bwd(1)")) return FOHO_ERR_LAUNCH;
        G = Gn;
    }
    return FOHO_OK;
}
