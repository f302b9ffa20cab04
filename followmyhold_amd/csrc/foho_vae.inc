// foho_vae.inc -- the ShapeVAE transformer of `latent2sdf` (PL:295 `pred = vae(pred)`), forward and backward to its input tokens, on the
// kernels of foho_geo.hip (included at its end: same translation unit, same GEMM / attention templates).
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

}  // namespace geo

// The attention backward of one image inside the chain (the split form: FOHO_VAE_SPLIT_DKV, or too few (head, key block) workgroups to
// fill the chip): like sdpa_bwd_image, with every streamed operand already there -- Qs, Qs^T, K^T from the forward's projection epilogue
// (EP_PACK), dO^T and delta from the epilogue of the GEMM that produced dO (EP_TRANS | EP_DELTA).
static int vae_attn_bwd_image(const SdpaLayout& l, char* base, const h16* qkv, int ld3, const h16* dO, const float* nls, h16* dqkv, const h16* qs, const h16* qst,
                              const h16* dot, int ldt, const h16* kt, const float* delta, int Lt, int heads, hipStream_t s) {
    const int W = heads * 64, nkb = Lt / 128;
    float* part = (float*)(base + l.part);
    const h16 *kb = qkv + W, *vb = qkv + 2 * W;
    const int splits = l.splits;
    hipLaunchKernelGGL(k_geo_attn_bwd, dim3(8 * ((heads * splits + 7) / 8) * nkb), dim3(256), 0, s, qs, qst, dO, dot, ldt, nls, delta, kb, ld3, W, heads, Lt, splits, Lt, 0, part,
                       (const int*)nullptr, vb, 64, (h16*)nullptr, (h16*)nullptr, ld3);
    const size_t n4 = (size_t)Lt * 2 * W / 4;
    hipLaunchKernelGGL(k_geo_dkv_reduce16, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, part, splits, Lt, W, dqkv + W, dqkv + 2 * W, ld3);
    hipLaunchKernelGGL(k_geo_attn_dq, dim3(((Lt + DQQ - 1) / DQQ) * heads), dim3(256), 0, s, qs, dO, W, kb, ld3, W, kt, Lt, nls, delta, dqkv, Lt, heads, vb, 64, ld3);
    return launch_ok("vae attention backward (split)") ? FOHO_OK : FOHO_ERR_LAUNCH;
}

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
    hipLaunchKernelGGL(k_vae_rowstat, dim3((M + 3) / 4), dim3(256), 0, s, X, M, W, d->layers[0].eps1, rowstat);
    if (!launch_ok("k_vae_rowstat")) return FOHO_ERR_LAUNCH;
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
        EpiAux aq;
        aq.vt = vtB, aq.lt = Lt, aq.ldqst = M, aq.qscale = SDPA_QSCALE;
        if (rec) aq.qs = (h16*)(rec + sv.qs), aq.qst = (h16*)(rec + sv.qst), aq.kt = (h16*)(rec + sv.kt);
        const int epq = EP_PREAFF | EP_PACK | (y.qk_norm ? EP_QKN : 0) | (PRE ? EP_SAVEZ : 0);
        if (int rc = gemm(epq, X, W, (const h16*)y.w_qkv, W, y.fold_qkv, (const h16*)rowstat, 3 * W, QKV, 3 * W, M, 3 * W, W, 1.0f, s, PRE, 3 * W, nullptr, GV_AUTO, aq)) return rc;
        {   // all images in ONE launch (blockIdx.y = image): 192 workgroups per image do not fill the chip
            const long i3 = (long)Lt * 3 * W, iw = (long)Lt * W;
            AttnB ab;
            ab.a = i3, ab.b = i3, ab.c = (long)W * Lt, ab.d = iw, ab.e = (long)Lt * NH;
            launch_attn(dim3(((Lt + AQ - 1) / AQ) * NH, B), s, QKV, 3 * W, QKV + W, 3 * W, (const h16*)vtB, Lt, O, W, Lt, NH, NLSE, (const int*)nullptr, 64, 64, SDPA_QSCALE,
                        (float*)nullptr, ab);
        }
        if (!launch_ok("foho_vae_fwd (attention)")) return FOHO_ERR_LAUNCH;
        if (int rc = gemm(EP_RESID | EP_STATS, O, W, (const h16*)y.w_proj, W, y.b_proj, X, W, X1, W, M, W, W, 1.0f, s, (h16*)stats, parts)) return rc;
        hipLaunchKernelGGL(k_geo_rowstat_finish, dim3((M + 15) / 16), dim3(256), 0, s, stats, parts, M, y.eps2, rowstat, (const int*)nullptr);
        if (!launch_ok("k_geo_rowstat_finish")) return FOHO_ERR_LAUNCH;
        if (int rc = gemm(EP_GELU | EP_PREAFF | (Z ? EP_SAVEZ : 0), X1, W, (const h16*)y.w_fc1, W, y.fold_fc1, (const h16*)rowstat, F, H, F, M, F, W, 1.0f, s, Z, Z ? F : 0))
            return rc;
        if (int rc = gemm(last ? EP_RESID : (EP_RESID | EP_STATS), H, F, (const h16*)y.w_fc2, F, y.b_fc2, X1, W, Xn, W, M, W, F, 1.0f, s, last ? nullptr : (h16*)stats,
                          last ? 0 : parts))
            return rc;
        if (!last) {
            hipLaunchKernelGGL(k_geo_rowstat_finish, dim3((M + 15) / 16), dim3(256), 0, s, stats, parts, M, d->layers[i + 1].eps1, rowstat, (const int*)nullptr);
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
    const float* nof = nullptr;
    const float* nog = nullptr;   // gamma = 1: the gradients come through the folded weights
    const dim3 rows((M + 3) / 4), blk(256);
    const h16* G = (const h16*)grad_out;
    for (int i = n - 1; i >= 0; i--) {
        const foho_vae_layer& y = d->layers[i];
        const char* rec = keep + (size_t)i * sv.per_layer;
        const h16 *X = (const h16*)(rec + sv.x), *QKV = (const h16*)(rec + sv.qkv), *PRE = (const h16*)(rec + sv.pre), *O = (const h16*)(rec + sv.o);
        const h16 *X1 = (const h16*)(rec + sv.x1), *Z = (const h16*)(rec + sv.z);
        const float* NLSE = (const float*)(rec + sv.nlse);
        const h16 *qsB = (const h16*)(rec + sv.qs), *QsT = (const h16*)(rec + sv.qst), *ktB = (const h16*)(rec + sv.kt);
        h16* Gn = (i == 0) ? (h16*)grad_x0 : GB;
        if (int rc = gemm(EP_GELUBWD, G, W, (const h16*)y.w_fc2_t, W, d->zeros, Z, F, H, F, M, F, W, 1.0f, s)) return rc;           // dZ
        if (int rc = gemm(0, H, F, (const h16*)y.w_fc1_t, F, d->zeros, nullptr, 0, T1, W, M, W, F, 1.0f, s)) return rc;             // d / d xhat of ln_2
        hipLaunchKernelGGL(k_geo_ln_bwd<0>, rows, blk, 0, s, X1, nog, (const h16*)T1, G, nof, 0.0f, nof, G1, M, W, y.eps2, (const int*)nullptr);
        if (!launch_ok("k_geo_ln_bwd(2)")) return FOHO_ERR_LAUNCH;
        EpiAux ad;
        ad.ndelta = deltaB, ad.heads = NH;
        if (int rc = gemm(EP_TRANS | EP_DELTA, G1, W, (const h16*)y.w_proj_t, W, d->zeros, O, W, dO, W, M, W, W, 1.0f, s, dOT, M, nullptr, GV_AUTO, ad)) return rc;   // dO, dO^T, delta
        if (direct) {   // all images in one launch per kernel (blockIdx.y / .z = image)
            const long i3 = (long)Lt * 3 * W, iw = (long)Lt * W, ih = (long)Lt * NH, it = (long)W * Lt;
            const int nkb = Lt / 128;
            AttnB bk, dq;
            bk.a = iw, bk.b = Lt, bk.c = iw, bk.d = Lt, bk.e = ih, bk.f = ih, bk.g = i3, bk.h = i3;
            dq.a = iw, dq.b = iw, dq.c = i3, dq.d = it, dq.e = ih, dq.f = ih, dq.g = i3;
            hipLaunchKernelGGL(k_geo_attn_bwd, dim3(8 * ((NH + 7) / 8) * nkb, B), blk, 0, s, qsB, QsT, (const h16*)dO, (const h16*)dOT, M, NLSE, (const float*)deltaB, QKV + W, 3 * W, W, NH,
                               Lt, 1, Lt, 0, (float*)nullptr, (const int*)nullptr, QKV + 2 * W, 64, dQKV + W, dQKV + 2 * W, 3 * W, bk);
            hipLaunchKernelGGL(k_geo_attn_dq, dim3(((Lt + DQQ - 1) / DQQ) * NH, B), blk, 0, s, qsB, (const h16*)dO, W, QKV + W, 3 * W, W, ktB, Lt, NLSE, (const float*)deltaB, dQKV, Lt, NH,
                               QKV + 2 * W, 64, 3 * W, dq);
            if (!launch_ok("vae attention backward")) return FOHO_ERR_LAUNCH;
        } else {
            for (int b = 0; b < B; b++) {
                const size_t r0 = (size_t)b * Lt;
                if (int rc = vae_attn_bwd_image(l.sl, base + l.sdpa, QKV + r0 * 3 * W, 3 * W, dO + r0 * W, NLSE + r0 * NH, dQKV + r0 * 3 * W, qsB + r0 * W, QsT + r0, dOT + r0, M,
                                                ktB + (size_t)b * W * Lt, deltaB + r0 * NH, Lt, NH, s))
                    return rc;
            }
        }
        if (y.qk_norm) {   // (inside the two kernels' way out it cost them 6-9 us each against the 8 us of this launch: NOTEBOOK round 6)
            const size_t lanes = (size_t)M * 2 * NH * 8;
            hipLaunchKernelGGL(k_vae_qknorm_bwd, dim3((unsigned)((lanes + 255) / 256)), blk, 0, s, dQKV, PRE, M, NH, y.fold_qkv + 6 * W);
            if (!launch_ok("k_vae_qknorm_bwd")) return FOHO_ERR_LAUNCH;
        }
        if (int rc = gemm(0, dQKV, 3 * W, (const h16*)y.w_qkv_t, 3 * W, d->zeros, nullptr, 0, T1, W, M, W, 3 * W, 1.0f, s)) return rc;   // d / d xhat of ln_1
        hipLaunchKernelGGL(k_geo_ln_bwd<0>, rows, blk, 0, s, X, nog, (const h16*)T1, (const h16*)G1, nof, 0.0f, nof, Gn, M, W, y.eps1, (const int*)nullptr);
        if (!launch_ok("k_geo_ln_bwd(1)")) return FOHO_ERR_LAUNCH;
        G = Gn;
    }
    return FOHO_OK;
}
