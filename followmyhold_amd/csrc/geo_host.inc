// geo_host.inc -- the host side of foho_geo.hip (included behind its kernels, in front of foho_vae.inc): for every kernel ONE function
// that launches it, gemm() with its typed epilogue description, the workspace layouts and the entry points of the geometry decoder
// (foho_geo_*), of the stand-alone attention (foho_sdpa_*) and the two unit entry points.
//
// Rules of this file (DESIGN.md section 7 has the how-to):
//   * a kernel is named in exactly one hipLaunchKernelGGL.  Its launcher owns the grid formula the kernel's block decoding relies on and
//     the conventions of the kernel's slots (the order of AttnB's a .. h, a null Vp, ...); callers name operands, never positions;
//   * what a GEMM epilogue needs is said with Epi's builders, which set the EP_* bit and its operands together, in the operands' own
//     types.  Only they know that the R / C2 / ldc2 slots of the kernels carry different things under different masks.

namespace geo {

// eps of one of the chain's LayerNorms: its own field when set, else ln_eps (callers of ABI 103 filled only that one)
static inline float eps_of(const foho_geo_weights* w, float own) { return own > 0.0f ? own : w->ln_eps; }
static bool launch_ok(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return false;
    }
    return true;
}
// what the attention kernels want folded into Q: log2(e) / sqrt(64) (they exponentiate with exp2)
static const float QSCALE = 1.4426950408889634f * 0.125f;

// ------------------------------------------------------------------------------------------------ GEMM
// Which kernel a GEMM runs on.  GV_AUTO: by shape (gemm() below); the others are for the unit entry point foho_geo_gemm (tests, A/B
// measurements) -- an ARGUMENT of the call, no process state: the library is driven from several threads (MeshGuidanceRunner, call_batch).
enum {
    GV_AUTO = 0,
    GV_128 = 1,         // k_geo_gemm: 128 x 128 tiles, two stages
    GV_LOCKSTEP = 2,    // k_geo_gemm256
    GV_PHASED = 3,      // k_geo_gemm8p, 256 x 256 tiles
    GV_DEEP = 4,        // k_geo_gemm_d4: 128 x 128 tiles, four-deep ring
    GV_PC = 5,          // k_geo_gemm_pc: the same with fill waves and matrix waves
    GV_PHASED192 = 6    // k_geo_gemm8p on 192 x 256 tiles
};
static unsigned cu_count() {   // a multiple of 8: the tile order deals consecutive tiles to the 8 XCDs
    static const unsigned ncu = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
        return (unsigned)(n & ~7);
    }();
    return ncu;
}

// The matrix operands: C (M, N) = epilogue(scale (A (M, K) . Wt (N, K)^T)).  Mdev: optional DEVICE row count (the launch is sized for M, the
// kernel works on min(M, *Mdev) rows).  variant: GV_*.
struct Gemm {
    const h16 *A = nullptr, *Wt = nullptr;
    h16* C = nullptr;
    int lda = 0, ldw = 0, ldc = 0, M = 0, N = 0, K = 0;
    float scale = 1.0f;
    const int* Mdev = nullptr;
    int variant = GV_AUTO;
};
// ... all three of them dense, which is every product of the chains.  Wt: a weight matrix as the ABI structs hold it (fp16).
static Gemm dense(const h16* A, const void* Wt, h16* C, int M, int N, int K, const int* Mdev = nullptr) {
    Gemm g;
    g.A = A, g.Wt = (const h16*)Wt, g.C = C, g.lda = g.ldw = K, g.ldc = N, g.M = M, g.N = N, g.K = K, g.Mdev = Mdev;
    return g;
}

// The epilogue of a GEMM: the EP_* mask (foho_geo.hip explains each bit) and its operands as the kernels take them.  Built from the bias
// vector by the functions below, each of which sets its bit and its operands together: Epi(b).resid(X, ld).stats(st, parts).
// The kernels have ONE slot R / ldr for what an epilogue reads per row and ONE slot C2 / ldc2 for what it writes besides C; no two
// builders that fill the same slot occur in one instantiated mask (gemm()'s switch).
struct Epi {
    int ep = 0;
    const float* bias;          // N floats; more under preaff() and logit()
    const h16* R = nullptr;
    int ldr = 0;
    h16* C2 = nullptr;
    int ldc2 = 0;
    EpiAux aux;
    explicit Epi(const float* b) : bias(b) {}
    Epi& gelu() { return ep |= EP_GELU, *this; }
    Epi& resid(const h16* X, int ld) { return ep |= EP_RESID, R = X, ldr = ld, *this; }             // C = ... + X
    Epi& gelu_bwd(const h16* Z, int ld) { return ep |= EP_GELUBWD, R = Z, ldr = ld, *this; }        // C = ... gelu'(Z), Z the saved pre-activation
    Epi& save_z(h16* Z, int ld) { return ep |= EP_SAVEZ, C2 = Z, ldc2 = ld, *this; }                // the pre-activation (EP_QKN: the un-normalised projection) -> Z
    Epi& trans(h16* Ct, int ldt) { return ep |= EP_TRANS, C2 = Ct, ldc2 = ldt, *this; }             // Ct[n][pos(m)], row length ldt
    Epi& qnorm(const float* qn) { return ep |= EP_QNORM, R = (const h16*)qn, ldr = 0, *this; }      // qn: gain (64), bias (64), eps
    // per row and 64-column part of the output (mean, M2): `parts` = N / 64 records of 2 floats per row
    Epi& stats(float* st, int parts) { return ep |= EP_STATS, C2 = (h16*)st, ldc2 = parts, *this; }
    // C is not stored; per row and part (mean, M2, row . gw): records of 4 floats.  bias: b (N) | gw (N)
    Epi& logit(float* st, int parts) { return ep |= EP_LOGIT, C2 = (h16*)st, ldc2 = parts, *this; }
    // LayerNorm folded into the weights: rowstat = (rstd, rstd mean) per row.  bias: b' (N) | s (N), and with qkn (N = 3 width: q | k | v)
    // behind them q_norm's and k_norm's gain (64), bias (64), eps in 132 floats each
    Epi& preaff(const float2* rowstat, int N, bool qkn = false) { return ep |= EP_PREAFF | (qkn ? EP_QKN : 0), R = (const h16*)rowstat, ldr = N, *this; }
    // the copies the attention kernels stream, of q | k | v: V^T, scaled Q, its transpose (row length ldqst), K^T; lt tokens per image.  Any may be null.
    Epi& pack(h16* vt, h16* qs, h16* qst, h16* kt, int lt, int ldqst, float qscale) {
        return ep |= EP_PACK, aux.vt = vt, aux.qs = qs, aux.qst = qst, aux.kt = kt, aux.lt = lt, aux.ldqst = ldqst, aux.qscale = qscale, *this;
    }
    // with trans(): ndelta[m][head] = -(C . O) per head, O the attention's output
    Epi& delta(const h16* O, int ldo, float* ndelta, int heads) { return ep |= EP_DELTA, R = O, ldr = ldo, aux.ndelta = ndelta, aux.heads = heads, *this; }
};

template <int EP>
static void launch_gemm(int variant, dim3 grid, hipStream_t s, const Gemm& g, const Epi& e) {
#define GEO_GEMM_ARGS g.A, g.lda, g.Wt, g.ldw, e.bias, e.R, e.ldr, g.C, g.ldc, g.M, g.N, g.K, g.scale, e.C2, e.ldc2, g.Mdev, e.aux
    if (variant == GV_PHASED192) hipLaunchKernelGGL((k_geo_gemm8p<EP, 192>), dim3(std::min(grid.x, cu_count())), dim3(512), 0, s, GEO_GEMM_ARGS);
    else if (variant == GV_PHASED) hipLaunchKernelGGL(k_geo_gemm8p<EP>, dim3(std::min(grid.x, cu_count())), dim3(512), 0, s, GEO_GEMM_ARGS);   // persistent: one workgroup per CU walks the tiles
    else if (variant == GV_PC) hipLaunchKernelGGL(k_geo_gemm_pc<EP>, grid, dim3(512), 0, s, GEO_GEMM_ARGS);
    else if (variant == GV_DEEP) hipLaunchKernelGGL(k_geo_gemm_d4<EP>, grid, dim3(256), 0, s, GEO_GEMM_ARGS);
    else if (variant == GV_LOCKSTEP) hipLaunchKernelGGL(k_geo_gemm256<EP>, grid, dim3(512), 0, s, GEO_GEMM_ARGS);
    else hipLaunchKernelGGL(k_geo_gemm<EP>, grid, dim3(256), 0, s, GEO_GEMM_ARGS);
#undef GEO_GEMM_ARGS
}

static int gemm(const Gemm& g, const Epi& e, hipStream_t s) {
    const int ep = e.ep, M = g.M, N = g.N, K = g.K;
    const EpiAux& aux = e.aux;
    if (M <= 0) return FOHO_OK;
    if (N % GN || K % GK || (g.lda & 7) || (g.ldw & 7) || (g.ldc & 7) || (e.R && !(ep & (EP_QNORM | EP_PREAFF)) && (e.ldr & 7)))
        return fail(FOHO_ERR_BAD_ARG, "geo gemm: N % 128, K % 64, leading dimensions % 8");
    if (((ep & EP_PREAFF) && e.ldr != N) || ((ep & (EP_STATS | EP_LOGIT)) && e.ldc2 * 64 != N) || ((ep & EP_QKN) && N % 192))
        return fail(FOHO_ERR_BAD_ARG, "geo gemm: folded-LayerNorm epilogue operands");
    const bool can_big = N % HN == 0 && K >= 256;
    // the phased kernel addresses its operands through 32-bit buffer offsets
    const bool can_phased = can_big && K / GK >= 2 && (size_t)M * g.lda * 2 < ((size_t)1 << 31) && (size_t)N * g.ldw * 2 < ((size_t)1 << 31);
    // the big GEMMs of the chain: 256 x 256 tiles -- when there are enough of them to occupy half the chip.  The ShapeVAE transformer's
    // N = 1024 products at M = 3072 are 48 such tiles on 256 CUs: 21 / 66 / 50 us at K = 1024 / 4096 / 3072 against 13 / 43 / 35 on 192 tiles of
    // 128 x 128 (scripts/dev/vae_bench.py --gemms)
    const long tiles256 = (long)((M + HM - 1) / HM) * (N / HN);
    const bool auto_choice = g.variant == GV_AUTO;
    int variant = g.variant;
    if (variant == GV_AUTO) variant = (can_big && M >= 2048 && tiles256 >= 128) ? (can_phased ? GV_PHASED : GV_LOCKSTEP) : GV_128;
    if ((variant == GV_PHASED || variant == GV_PHASED192) && !can_phased) variant = can_big ? GV_LOCKSTEP : GV_128;
    // 256-row tiles whose last round leaves CUs idle (the transformer's M = 3072: 12 x 16 tiles on 256 CUs; four images' q | k | v: 2.25 rounds) ->
    // 192-row tiles when the busiest CU then multiplies fewer rows: rounds x rows per tile, 192-row rounds counted 8 % dearer (their phases 1 and 2
    // run four matrix instructions behind the same two barriers; the decoder's 49 152-row blocks are exact rounds either way and stay)
    if (variant == GV_PHASED && auto_choice && M > 192 && !((ep & EP_PACK) && aux.lt % 192)) {
        const long cu = (long)cu_count();
        const long t256 = 8L * (((M + HM - 1) / HM + 7) / 8) * (N / HN), t192 = 8L * (((M + 191) / 192 + 7) / 8) * (N / HN);
        if (((t192 + cu - 1) / cu) * 192 * 108 < ((t256 + cu - 1) / cu) * 256 * 100) variant = GV_PHASED192;
    }
    if (variant == GV_LOCKSTEP && !can_big) variant = GV_128;
    // 128 x 128 tiles that do not even fill the chip once: one workgroup per CU, and with one wave per SIMD the ring's fill and the matrix
    // work add up (NOTEBOOK round 6) -> the eight-wave kernel whose waves 4-7 fill while waves 0-3 multiply
    if (variant == GV_128 && auto_choice && 8L * (((M + GM - 1) / GM + 7) / 8) * (N / GN) <= (long)cu_count() && K / GK >= 4) variant = GV_PC;
    if ((ep & EP_PACK) && (!(ep & EP_PREAFF) || N % 3 || (N / 3) % 64 || M % 64 || aux.lt <= 0 || aux.lt % 64 || M % aux.lt || (aux.qst && aux.ldqst < M)))
        return fail(FOHO_ERR_BAD_ARG, "geo gemm: EP_PACK operands");
    if ((ep & EP_DELTA) && (!(ep & EP_TRANS) || !aux.ndelta || aux.heads * 64 != N)) return fail(FOHO_ERR_BAD_ARG, "geo gemm: EP_DELTA operands");
    if (variant == GV_PHASED192 && (ep & EP_PACK) && aux.lt % 192) variant = GV_PHASED;   // (a 32-row part would straddle two images)
    const bool big = variant != GV_128 && variant != GV_DEEP && variant != GV_PC;
    const int tn = big ? HN : GN, tm = variant == GV_PHASED192 ? 192 : (big ? HM : GM);
    const int ntn = N / tn, ntm = (M + tm - 1) / tm;
    const dim3 grid(8 * ((ntm + 7) / 8) * ntn);
#define GEO_GEMM_CASE(E) case E: launch_gemm<E>(variant, grid, s, g, e); break
    switch (ep) {
        GEO_GEMM_CASE(0);
        GEO_GEMM_CASE(EP_GELU);
        GEO_GEMM_CASE(EP_RESID);
        GEO_GEMM_CASE(EP_GELU | EP_SAVEZ);
        GEO_GEMM_CASE(EP_GELUBWD);
        GEO_GEMM_CASE(EP_TRANS);
        GEO_GEMM_CASE(EP_QNORM);
        GEO_GEMM_CASE(EP_TRANS | EP_QNORM);
        GEO_GEMM_CASE(EP_RESID | EP_STATS);
        GEO_GEMM_CASE(EP_GELU | EP_PREAFF);
        GEO_GEMM_CASE(EP_RESID | EP_LOGIT);
        // the ShapeVAE transformer's (foho_vae.inc): fused q | k | v behind a folded LayerNorm (+ qk_norm, + the un-normalised copy), fc1 keeping its pre-activation
        // (+ EP_PACK: the transposed / scaled copies the attention kernels stream; EP_TRANS | EP_DELTA: dO, dO^T and the backward's delta)
        GEO_GEMM_CASE(EP_PREAFF | EP_PACK);
        GEO_GEMM_CASE(EP_PREAFF | EP_QKN | EP_PACK);
        GEO_GEMM_CASE(EP_PREAFF | EP_QKN | EP_SAVEZ | EP_PACK);
        GEO_GEMM_CASE(EP_GELU | EP_PREAFF | EP_SAVEZ);
        GEO_GEMM_CASE(EP_TRANS | EP_DELTA);
        default: return fail(FOHO_ERR_BAD_ARG, "geo gemm: epilogue");
    }
#undef GEO_GEMM_CASE
    return launch_ok("k_geo_gemm") ? FOHO_OK : FOHO_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ row kernels: one wave per row
// Y = LN(X) gamma + beta
static void ln_rows(hipStream_t s, const h16* X, int ldx, const float* gamma, const float* beta, float eps, h16* Y, int ldy, int M, int width, const int* Mdev = nullptr) {
    const float* nof = nullptr;
    hipLaunchKernelGGL(k_geo_ln<0>, dim3((M + 3) / 4), dim3(256), 0, s, X, ldx, gamma, beta, Y, ldy, M, width, eps, nof, 0.0f, nof, 0.0f, 0.0f, 0.0f, (float*)nullptr, Mdev);
}
// logits = output_proj(ln_post(X2)) (+ the stand-in's analytic prior of the query points q)
static void ln_logits(hipStream_t s, const foho_geo_weights* w, const h16* X2, const float* q, int M, float* logits) {
    hipLaunchKernelGGL(k_geo_ln<1>, dim3((M + 3) / 4), dim3(256), 0, s, X2, w->width, w->ln_post_g, w->ln_post_b, (h16*)nullptr, 0, M, w->width, w->ln_eps, w->w_out,
                       w->b_out, q, w->prior_radius, w->prior_sharpness, w->out_gain, logits, (const int*)nullptr);
}
// ... its backward: dX2 from the logits' gradient
static void ln_logits_bwd(hipStream_t s, const foho_geo_weights* w, const h16* X2, const float* grad_logits, h16* dX2, int M, const int* Mdev) {
    hipLaunchKernelGGL(k_geo_ln_bwd<1>, dim3((M + 3) / 4), dim3(256), 0, s, X2, w->ln_post_g, (const h16*)nullptr, (const h16*)nullptr, grad_logits, w->out_gain, w->w_out,
                       dX2, M, w->width, w->ln_eps, Mdev);
}
// DX = (DR ? DR : 0) + LayerNorm'(X; DY); gamma == NULL: all ones
static void ln_rows_bwd(hipStream_t s, const h16* X, const float* gamma, float eps, const h16* DY, const h16* DR, h16* DX, int M, int width, const int* Mdev = nullptr) {
    const float* nof = nullptr;
    hipLaunchKernelGGL(k_geo_ln_bwd<0>, dim3((M + 3) / 4), dim3(256), 0, s, X, gamma, DY, DR, nof, 0.0f, nof, DX, M, width, eps, Mdev);
}
static void embed(hipStream_t s, const foho_geo_weights* w, const float* q, int M, h16* E, const int* Mdev) {   // 8 lanes per row
    hipLaunchKernelGGL(k_geo_embed, dim3((M * 8 + 255) / 256), dim3(256), 0, s, q, M, w->n_freqs, w->freqs, E, Mdev);
}
// the row statistics an EP_STATS epilogue left in `stats` -> (rstd, rstd mean) per row; 16 lanes per row
static void rowstat_finish(hipStream_t s, const float* stats, int parts, int M, float eps, float2* rowstat, const int* Mdev = nullptr) {
    hipLaunchKernelGGL(k_geo_rowstat_finish, dim3((M + 15) / 16), dim3(256), 0, s, stats, parts, M, eps, rowstat, Mdev);
}
// ... what an EP_LOGIT epilogue left there -> logits; gwc0 = (GW, C0), the tail of fold2
static void logit_finish(hipStream_t s, const foho_geo_weights* w, const float* stats, int parts, int M, const float* gwc0, const float* q, float* logits, const int* Mdev) {
    hipLaunchKernelGGL(k_geo_logit_finish, dim3((M + 15) / 16), dim3(256), 0, s, stats, parts, M, w->ln_eps, gwc0, w->b_out, q, w->prior_radius, w->prior_sharpness,
                       w->out_gain, logits, Mdev);
}
// ndelta of the rows up to the next multiple of 64 (the padding of the last query tile gets 0)
static void delta(hipStream_t s, const h16* dO, const h16* O, int width, int heads, int M, float* ndelta, const int* Mdev = nullptr) {
    hipLaunchKernelGGL(k_geo_delta, dim3((((M + 63) & ~63) + 3) / 4), dim3(256), 0, s, dO, O, width, heads, M, ndelta, Mdev);
}
static void knorm(hipStream_t s, h16* KV, int ldkv, int L, int heads, const float* kn) {   // one thread per (token, head)
    hipLaunchKernelGGL(k_geo_knorm, dim3((L * heads + 255) / 256), dim3(256), 0, s, KV, ldkv, L, heads, kn);
}

// ------------------------------------------------------------------------------------------------ what the attention kernels stream
// Vt[head][d][pos(l)] of the `width` columns of X (L rows of stride ldx) that start at col0 -- default: at `width`, the V half of a K | V
// projection --, heads hs apart; one thread per (column, 16 keys)
static void pack_vt(hipStream_t s, const h16* X, int ldx, int width, int L, h16* Vt, int col0 = -1, int hs = 64) {
    hipLaunchKernelGGL(k_geo_pack_vt, dim3((width + 255) / 256, L / 16), dim3(256), 0, s, X, ldx, width, L, Vt, col0, hs);
}
// XT[c][pos(m)] (row length ldt) of X (M rows of stride ldx, heads hs apart); scale != 1: of the scaled X, which also goes to Xs (M, W)
static void transpose_perm(hipStream_t s, const h16* X, int ldx, int M, int W, h16* XT, int ldt, int hs = 64, float scale = 1.0f, h16* Xs = nullptr) {
    hipLaunchKernelGGL(k_geo_transpose_perm, dim3((unsigned)(((size_t)M * (W / 8) + 255) / 256)), dim3(256), 0, s, X, ldx, M, W, XT, ldt, hs, scale, Xs);
}
// n halfs (a multiple of 8) of zeros, by a kernel: where the call must be capturable in a graph (memset nodes are not reliably ordered on this stack)
static void zero16(hipStream_t s, h16* p, size_t n) {
    const size_t n16 = n * 2 / 16;
    hipLaunchKernelGGL(k_geo_zero16, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, (uint4*)p, n16);
}

// ------------------------------------------------------------------------------------------------ attention
// Per-image strides of a batched launch (the image is blockIdx.y): by operand, in elements of the operand; all 0 with images == 1.  The
// launchers alone know which letter of AttnB a kernel reads for which operand.
//
// Forward: O (M, heads x 64; stride ldo) = softmax(Q K^T) V.  Q rows of stride ldq, K rows of stride ldk, heads qhs / khs apart; Vt from pack_vt.
// qscale != 1: Q arrives unscaled (else: with QSCALE folded in).  nlse: optional -lse (log2 domain, for the backward), lse_nat: optional natural-log lse.
struct AttnFwd {
    const h16 *Q = nullptr, *K = nullptr, *Vt = nullptr;
    h16* O = nullptr;
    int ldq = 0, ldk = 0, ldo = 0, qhs = 64, khs = 64, M = 0, L = 0, heads = 0, images = 1;
    float qscale = 1.0f;
    float *nlse = nullptr, *lse_nat = nullptr;
    const int* Mdev = nullptr;
    struct {
        long q = 0, k = 0, vt = 0, o = 0, nlse = 0, lse_nat = 0;
    } img;
};
static void attn_fwd(hipStream_t s, const AttnFwd& a) {
    AttnB bs;
    bs.a = a.img.q, bs.b = a.img.k, bs.c = a.img.vt, bs.d = a.img.o, bs.e = a.img.nlse, bs.f = a.img.lse_nat;
    hipLaunchKernelGGL(k_geo_attn, dim3(((a.M + AQ - 1) / AQ) * a.heads, a.images), dim3(256), 0, s, a.Q, a.ldq, a.K, a.ldk, a.Vt, a.L, a.O, a.ldo, a.M, a.heads, a.nlse, a.Mdev,
                       a.qhs, a.khs, a.qscale, a.lse_nat, bs);
}

// dK, dV: Qs (M, width) and dO (M, width) and their transposes QsT / dOT (row length ldt), -lse and -delta per (row, head); K rows at
// KV + key ldkv + head khs, V rows at Vp + ... (Vp == nullptr: KV + width, the V half of a K | V projection).
// dk16 / dv16 set (rows of stride ld16): the direct route -- splits == 1, every workgroup writes its dK / dV itself, images side by side in
// one launch.  Else fp32 partial sums of `splits` workgroups per (head, key block) go to `part` (accumulate: added to what is there),
// one image per launch.
struct AttnBwd {
    const h16 *Qs = nullptr, *QsT = nullptr, *dO = nullptr, *dOT = nullptr, *KV = nullptr, *Vp = nullptr;
    const float *nlse = nullptr, *ndelta = nullptr;
    int ldt = 0, ldkv = 0, khs = 64, width = 0, heads = 0, M = 0, L = 0, splits = 1, accumulate = 0, images = 1;
    float* part = nullptr;
    const int* Mdev = nullptr;
    h16 *dk16 = nullptr, *dv16 = nullptr;
    int ld16 = 0;
    struct {
        long qs = 0, qst = 0, dO = 0, dOT = 0, nlse = 0, ndelta = 0, kv = 0, dkv = 0;
    } img;
};
static void attn_bwd(hipStream_t s, const AttnBwd& a) {
    AttnB bs;
    bs.a = a.img.qs, bs.b = a.img.qst, bs.c = a.img.dO, bs.d = a.img.dOT, bs.e = a.img.nlse, bs.f = a.img.ndelta, bs.g = a.img.kv, bs.h = a.img.dkv;
    // a (head, split) group's L / 128 workgroups on consecutive slots of ONE XCD: groups rounded up to a multiple of 8
    hipLaunchKernelGGL(k_geo_attn_bwd, dim3(8 * ((a.heads * a.splits + 7) / 8) * (a.L / 128), a.images), dim3(256), 0, s, a.Qs, a.QsT, a.dO, a.dOT, a.ldt, a.nlse, a.ndelta, a.KV,
                       a.ldkv, a.width, a.heads, a.M, a.splits, a.L, a.accumulate, a.part, a.Mdev, a.Vp, a.khs, a.dk16, a.dv16, a.ld16, bs);
}
// dQ (rows of stride lddq; 0: ldq, that of Qs and dO): K / V rows as above, Kt = K^T from pack_vt
struct AttnDq {
    const h16 *Qs = nullptr, *dO = nullptr, *KV = nullptr, *Vp = nullptr, *Kt = nullptr;
    const float *nlse = nullptr, *ndelta = nullptr;
    h16* dQ = nullptr;
    int ldq = 0, ldkv = 0, khs = 64, lddq = 0, width = 0, heads = 0, M = 0, L = 0, images = 1;
    struct {
        long qs = 0, dO = 0, kv = 0, kt = 0, nlse = 0, ndelta = 0, dq = 0;
    } img;
};
static void attn_dq(hipStream_t s, const AttnDq& a) {
    AttnB bs;
    bs.a = a.img.qs, bs.b = a.img.dO, bs.c = a.img.kv, bs.d = a.img.kt, bs.e = a.img.nlse, bs.f = a.img.ndelta, bs.g = a.img.dq;
    hipLaunchKernelGGL(k_geo_attn_dq, dim3(((a.M + DQQ - 1) / DQQ) * a.heads, a.images), dim3(256), 0, s, a.Qs, a.dO, a.ldq, a.KV, a.ldkv, a.width, a.Kt, a.L, a.nlse, a.ndelta, a.dQ,
                       a.M, a.heads, a.Vp, a.khs, a.lddq, bs);
}
// image i of a batched description, as a launch of its own
static AttnBwd image_of(AttnBwd a, int i) {
    a.Qs += i * a.img.qs, a.QsT += i * a.img.qst, a.dO += i * a.img.dO, a.dOT += i * a.img.dOT, a.nlse += i * a.img.nlse, a.ndelta += i * a.img.ndelta, a.KV += i * a.img.kv;
    if (a.Vp) a.Vp += i * a.img.kv;
    a.dk16 += i * a.img.dkv, a.dv16 += i * a.img.dkv, a.images = 1;
    return a;
}
static AttnDq image_of(AttnDq a, int i) {
    a.Qs += i * a.img.qs, a.dO += i * a.img.dO, a.KV += i * a.img.kv, a.Kt += i * a.img.kt, a.nlse += i * a.img.nlse, a.ndelta += i * a.img.ndelta, a.dQ += i * a.img.dq;
    if (a.Vp) a.Vp += i * a.img.kv;
    a.images = 1;
    return a;
}
// the sum over the splits' partial sums (fixed order: bitwise repeatable) -> grad_kv (L, 2 width) fp32 ...
static int dkv_reduce(hipStream_t s, const float* part, int splits, int L, int width, float* grad_kv) {
    const size_t n4 = (size_t)L * 2 * width / 4;
    hipLaunchKernelGGL(k_geo_dkv_reduce, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, part, splits, n4, grad_kv);
    return launch_ok("k_geo_dkv_reduce") ? FOHO_OK : FOHO_ERR_LAUNCH;
}
// ... or -> dk, dv (L, width) fp16, rows of stride ld
static void dkv_reduce16(hipStream_t s, const float* part, int splits, int L, int width, h16* dk, h16* dv, int ld) {
    const size_t n4 = (size_t)L * 2 * width / 4;
    hipLaunchKernelGGL(k_geo_dkv_reduce16, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, part, splits, L, width, dk, dv, ld);
}
// The split route of one image's attention backward: `splits` workgroups per (head, key block) leave partial sums in `part`, the reduce
// writes dK / dV where b.dk16 / b.dv16 point, then dQ.  (Whether to take it is the caller's decision.)
static int attn_bwd_split(hipStream_t s, AttnBwd b, const AttnDq& q, int splits, float* part) {
    h16 *dk = b.dk16, *dv = b.dv16;
    b.dk16 = b.dv16 = nullptr, b.splits = splits, b.part = part;
    attn_bwd(s, b);
    dkv_reduce16(s, part, splits, b.L, b.width, dk, dv, b.ld16);
    attn_dq(s, q);
    return launch_ok("attention backward (split)") ? FOHO_OK : FOHO_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ the decoder's workspace
static int check_weights(const foho_geo_weights* w) {
    if (!w) return fail(FOHO_ERR_BAD_ARG, "foho_geo: null weights");
    if (w->width <= 0 || w->width % 128 || w->width > 1024) return fail(FOHO_ERR_BAD_ARG, "foho_geo: width must be a multiple of 128, at most 1024");
    if (w->heads <= 0 || w->width != w->heads * 64) return fail(FOHO_ERR_BAD_ARG, "foho_geo: head dimension must be 64");
    if (w->n_latents <= 0 || w->n_latents % 64) return fail(FOHO_ERR_BAD_ARG, "foho_geo: n_latents must be a multiple of 64");
    if (w->hidden <= 0 || w->hidden % 128) return fail(FOHO_ERR_BAD_ARG, "foho_geo: hidden must be a multiple of 128");
    if (w->n_freqs < 0 || w->n_freqs > 10) return fail(FOHO_ERR_BAD_ARG, "foho_geo: 3 (2 n_freqs + 1) must fit 64 columns");
    if ((size_t)w->n_latents * w->width * 4 >= ((size_t)1 << 31)) return fail(FOHO_ERR_BAD_ARG, "foho_geo: K / V of the latent tokens exceed 32-bit buffer offsets");
    if (!w->w_qproj || !w->b_qproj || !w->w_q || !w->b_q || !w->w_kv || !w->b_kv || !w->w_proj || !w->b_proj || !w->w_fc1 || !w->b_fc1 ||
        !w->w_fc2 || !w->b_fc2 || !w->w_out || !w->ln_q_g || !w->ln_q_b || !w->ln_kv_g || !w->ln_kv_b || !w->ln_2_g || !w->ln_2_b ||
        !w->ln_post_g || !w->ln_post_b || !w->freqs)
        return fail(FOHO_ERR_BAD_ARG, "foho_geo: null weight pointer");
    return FOHO_OK;
}

struct Layout {
    size_t kv, vt, e, a, b, c, h, w1f, fold1, fold2, stats, rowstat, total;
};
static Layout layout(const foho_geo_weights* w, int chunk) {
    Layout l{};
    Carve cv;
    const size_t W = w->width, F = w->hidden, C = chunk, Lr = w->n_latents, rows = std::max<size_t>(chunk, Lr);  // the prepare step normalises the latents in buffer A
    l.kv = cv.take(Lr * 2 * W * 2);
    l.vt = cv.take(W * Lr * 2);
    // LayerNorm folded into the forward GEMMs (chain_latent_side): fc1's weights with ln_2's gain and the folded vectors -- like kv / vt
    // written by the prepare step, at offsets that do not depend on the chunk
    l.w1f = cv.take(F * W * 2);
    l.fold1 = cv.take(2 * F * 4);               // 2 hidden floats
    l.fold2 = cv.take((2 * W + 4) * 4);         // 2 W + 2 floats, in room for 2 W + 4
    l.e = cv.take(C * 64 * 2);
    l.a = cv.take(rows * W * 2);
    l.b = cv.take(C * W * 2);
    l.c = cv.take(C * W * 2);
    l.h = cv.take(C * F * 2);
    // ... the per-row statistics of the folded LayerNorms (16 parts of 4 floats at width 1024) and (rstd, rstd mean) per row
    l.stats = cv.take(C * (W / 64) * 4 * 4);    // chunk x parts x 4 floats
    l.rowstat = cv.take(C * 2 * 4);             // chunk x 2 floats
    l.total = cv.off;
    return l;
}
struct Fold {   // device pointers of the folded operands in a prepared workspace (w1f == nullptr: chain with LayerNorm kernels)
    const h16* w1f = nullptr;
    const float *fold1 = nullptr, *fold2 = nullptr;
    float* stats = nullptr;
    float2* rowstat = nullptr;
};
static Fold fold_of(const foho_geo_weights* w, const Layout& l, char* base) {
    Fold f;
    if (w->flags & FOHO_GEO_NO_LNFUSE) return f;   // the forward chain with its LayerNorm kernels (A/B measurements, the parity test of the folded form)
    f.w1f = (const h16*)(base + l.w1f), f.fold1 = (const float*)(base + l.fold1), f.fold2 = (const float*)(base + l.fold2);
    f.stats = (float*)(base + l.stats), f.rowstat = (float2*)(base + l.rowstat);
    return f;
}
static int fold_weights(const foho_geo_weights* w, const Layout& l, char* base, hipStream_t s) {
    const int W = w->width, F = w->hidden;
    hipLaunchKernelGGL(k_geo_fold_fc1, dim3((F + 3) / 4), dim3(256), 0, s, (const h16*)w->w_fc1, w->b_fc1, w->ln_2_g, w->ln_2_b, F, W, (h16*)(base + l.w1f),
                       (float*)(base + l.fold1));
    hipLaunchKernelGGL(k_geo_fold_post, dim3(1), dim3(256), 0, s, w->b_fc2, w->ln_post_g, w->ln_post_b, w->w_out, W, (float*)(base + l.fold2));
    return launch_ok("k_geo_fold") ? FOHO_OK : FOHO_ERR_LAUNCH;
}

// A prepared workspace as an entry point sees it: its layout and the K | V projection and V^T of the latent tokens in it.
struct Ws {
    Layout l;
    char* base;
    h16 *kv, *vt;
};
static Ws ws_of(const foho_geo_weights* w, int chunk, void* ws) {
    Ws o{layout(w, chunk), (char*)ws, nullptr, nullptr};
    o.kv = (h16*)(o.base + o.l.kv), o.vt = (h16*)(o.base + o.l.vt);
    return o;
}
// The preamble of an entry point `who`: the weights, its own arguments (args_ok; it covers ws != NULL and chunk_rows > 0), the workspace's size.
static int open_ws(const char* who, const foho_geo_weights* w, bool args_ok, int chunk, void* ws, size_t ws_bytes, Ws& o) {
    if (int rc = check_weights(w)) return rc;
    if (!args_ok) return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": null argument");
    o = ws_of(w, chunk, ws);
    if (ws_bytes < o.l.total) return fail(FOHO_ERR_WORKSPACE, std::string(who) + ": workspace too small");
    return FOHO_OK;
}
// K | V of the latent tokens are in o.kv: V^T for the attention and the folded operands
static int finish_kv(const foho_geo_weights* w, const Ws& o, hipStream_t s) {
    pack_vt(s, o.kv, 2 * w->width, w->width, w->n_latents, o.vt);
    if (!launch_ok("k_geo_pack_vt")) return FOHO_ERR_LAUNCH;
    return fold_weights(w, o.l, o.base, s);
}

}  // namespace geo

using namespace geo;

extern "C" const char* foho_geo_last_error(void) { return g_err; }

extern "C" int64_t foho_geo_abi_size(void) { return (int64_t)sizeof(foho_geo_weights); }

extern "C" size_t foho_geo_workspace_bytes(const foho_geo_weights* w, int32_t chunk_rows) {
    if (check_weights(w) != FOHO_OK || chunk_rows <= 0) return 0;
    return layout(w, chunk_rows).total;
}

extern "C" int foho_geo_prepare(const foho_geo_weights* w, const void* latents, int32_t chunk_rows, void* ws, size_t ws_bytes, void* stream_) {
    Ws o;
    if (int rc = open_ws("foho_geo_prepare", w, latents && ws && chunk_rows > 0, chunk_rows, ws, ws_bytes, o)) return rc;
    hipStream_t s = (hipStream_t)stream_;
    h16* ln = (h16*)(o.base + o.l.a);
    const int W = w->width, Lr = w->n_latents;
    ln_rows(s, (const h16*)latents, W, w->ln_kv_g, w->ln_kv_b, eps_of(w, w->ln_kv_eps), ln, W, Lr, W);
    if (!launch_ok("k_geo_ln(kv)")) return FOHO_ERR_LAUNCH;
    if (int rc = gemm(dense(ln, w->w_kv, o.kv, Lr, 2 * W, W), Epi(w->b_kv), s)) return rc;
    if (w->k_norm) knorm(s, o.kv, 2 * W, Lr, w->heads, w->k_norm);
    return finish_kv(w, o, s);
}

// ---- the forward chain in two halves: what depends only on the query points (Fourier embedding -> query projection -> ln_q ->
// c_q [+ q_norm], scaled for the exp2 softmax), and what depends on the latent tokens.  The first half is the same for every
// decode of one grid (foho_geo_prepare_queries caches it: X0 and Qs of all rows, 4 KB per query at width 1024).
static int chain_query_side(const foho_geo_weights* w, const float* q, int M, h16* E, h16* X0, h16* Xn, h16* Qs, h16* QsT, int ldt, hipStream_t s,
                            const int* Mdev = nullptr) {
    const int W = w->width;
    embed(s, w, q, M, E, Mdev);
    if (!launch_ok("k_geo_embed")) return FOHO_ERR_LAUNCH;
    if (int rc = gemm(dense(E, w->w_qproj, X0, M, W, 64, Mdev), Epi(w->b_qproj), s)) return rc;
    ln_rows(s, X0, W, w->ln_q_g, w->ln_q_b, eps_of(w, w->ln_q_eps), Xn, W, M, W, Mdev);
    if (!launch_ok("k_geo_ln(q)")) return FOHO_ERR_LAUNCH;
    Gemm cq = dense(Xn, w->w_q, Qs, M, W, W, Mdev);
    cq.scale = QSCALE;
    Epi e(w->b_q);
    if (QsT) e.trans(QsT, ldt);
    if (w->q_norm) e.qnorm(w->q_norm);
    return gemm(cq, e, s);
}

// attention over the latent tokens -> c_proj + residual -> ln_2 -> fc1 + GELU -> fc2 + residual.  Z != NULL keeps the MLP's
// pre-activation, lse != NULL the attention's log-sum-exp (both for a backward).  X0 / Qs: the query side's outputs for these rows.
//
// With `fold` (the plain forward: nothing kept, logits wanted) the two LayerNorms of this half never run as kernels:
//   ln_2 -> fc1:  LN(x) W^T = rstd (x (W gamma)^T) - rstd mean s + (b + W beta), s = row sums of W gamma -- c_proj's epilogue leaves the
//     row statistics of x1 (EP_STATS), fc1 multiplies the un-normalised x1 with the folded weights and applies (rstd, mean) per row in
//     its epilogue in front of the GELU (EP_PREAFF);
//   fc2 -> ln_post -> output_proj:  logit = rstd (x2 . gw - mean GW) + C0 + b_out, gw = gamma_post w_out -- fc2's epilogue reduces its
//     rows to (mean, M2, x2 . gw) per 64-column part (EP_LOGIT) and x2 is never written; k_geo_logit_finish merges the parts.
// Same fp16-rounded x1 / x2 as the chain with LayerNorm kernels; what differs is one rounding (LN output to fp16 there, W gamma to
// fp16 here) -- tests/test_geo_decode.py compares the two forms.  100 MB of reads + 100 MB of writes less per LayerNorm and row block.
static int chain_latent_side(const foho_geo_weights* w, int M, const h16* X0, const h16* Qs, h16* At, h16* X1, h16* Xn, h16* Z, h16* H, h16* X2, float* lse,
                             const h16* kv, const h16* vt, hipStream_t s, const int* Mdev = nullptr, const Fold* fold = nullptr, const float* q = nullptr,
                             float* logits = nullptr) {
    const int W = w->width, Lr = w->n_latents, F = w->hidden, NH = w->heads;
    AttnFwd a;
    a.Q = Qs, a.ldq = W, a.K = kv, a.ldk = 2 * W, a.Vt = vt, a.L = Lr, a.O = At, a.ldo = W, a.M = M, a.heads = NH, a.nlse = lse, a.Mdev = Mdev;
    attn_fwd(s, a);
    if (!launch_ok("k_geo_attn")) return FOHO_ERR_LAUNCH;
    if (fold && fold->w1f && !Z) {
        const int parts = W / 64;
        if (int rc = gemm(dense(At, w->w_proj, X1, M, W, W, Mdev), Epi(w->b_proj).resid(X0, W).stats(fold->stats, parts), s)) return rc;
        rowstat_finish(s, fold->stats, parts, M, eps_of(w, w->ln_2_eps), fold->rowstat, Mdev);
        if (!launch_ok("k_geo_rowstat_finish")) return FOHO_ERR_LAUNCH;
        if (int rc = gemm(dense(X1, fold->w1f, H, M, F, W, Mdev), Epi(fold->fold1).gelu().preaff(fold->rowstat, F), s)) return rc;
        if (int rc = gemm(dense(H, w->w_fc2, X2, M, W, F, Mdev), Epi(fold->fold2).resid(X1, W).logit(fold->stats, parts), s)) return rc;
        logit_finish(s, w, fold->stats, parts, M, fold->fold2 + 2 * W, q, logits, Mdev);
        return launch_ok("k_geo_logit_finish") ? FOHO_OK : FOHO_ERR_LAUNCH;
    }
    if (int rc = gemm(dense(At, w->w_proj, X1, M, W, W, Mdev), Epi(w->b_proj).resid(X0, W), s)) return rc;
    ln_rows(s, X1, W, w->ln_2_g, w->ln_2_b, eps_of(w, w->ln_2_eps), Xn, W, M, W, Mdev);
    if (!launch_ok("k_geo_ln(2)")) return FOHO_ERR_LAUNCH;
    Epi fc1(w->b_fc1);
    fc1.gelu();
    if (Z) fc1.save_z(Z, F);
    if (int rc = gemm(dense(Xn, w->w_fc1, H, M, F, W, Mdev), fc1, s)) return rc;
    return gemm(dense(H, w->w_fc2, X2, M, W, F, Mdev), Epi(w->b_fc2).resid(X1, W), s);
}

// logits = output_proj(ln_post(x2)) (+ the stand-in's analytic prior)
static int chain_logits(const foho_geo_weights* w, const float* q, int M, const h16* X2, float* logits, hipStream_t s) {
    ln_logits(s, w, X2, q, M, logits);
    return launch_ok("k_geo_ln(post)") ? FOHO_OK : FOHO_ERR_LAUNCH;
}

extern "C" int foho_geo_decode_fwd(const foho_geo_weights* w, const float* queries, int64_t n_queries, float* logits, int32_t chunk_rows,
                                   void* ws, size_t ws_bytes, void* stream_) {
    Ws o;
    if (int rc = open_ws("foho_geo_decode_fwd", w, queries && logits && ws && chunk_rows > 0 && n_queries >= 0, chunk_rows, ws, ws_bytes, o)) return rc;
    hipStream_t s = (hipStream_t)stream_;
    const Layout& l = o.l;
    char* base = o.base;
    const h16 *kv = o.kv, *vt = o.vt;
    h16 *E = (h16*)(base + l.e), *bA = (h16*)(base + l.a), *bB = (h16*)(base + l.b), *bC = (h16*)(base + l.c), *bH = (h16*)(base + l.h);
    const Fold fold = fold_of(w, l, base);
    for (int64_t r0 = 0; r0 < n_queries; r0 += chunk_rows) {
        const int M = (int)std::min<int64_t>(chunk_rows, n_queries - r0);
        const float* q = queries + 3 * r0;
        // x0 -> A, ln_q(x0) -> B, q -> C;  attention C -> B;  x1 = x0 + c_proj: B (+A) -> C;  ln_2: C -> B;  fc1: B -> H;  x2 = x1 + fc2: H (+C) -> A
        if (int rc = chain_query_side(w, q, M, E, bA, bB, bC, nullptr, 0, s)) return rc;
        if (int rc = chain_latent_side(w, M, bA, bC, bB, bC, bB, nullptr, bH, bA, nullptr, kv, vt, s, nullptr, &fold, q, logits + r0)) return rc;
        if (!fold.w1f)
            if (int rc = chain_logits(w, q, M, bA, logits + r0, s)) return rc;
    }
    return FOHO_OK;
}

// ---- the query side, cached (PL:1125-1143, 298-308: the grid of a guidance run never changes -- 65^3 points for all 550 inner
// iterations of every image): X0 = query_proj(embed(q)) and Qs = c_q(ln_q(X0)) [q_norm] log2(e) / 8 of ALL rows, fp16.
struct CacheLayout {
    size_t x0, qs, total;
};
static CacheLayout cache_layout(const foho_geo_weights* w, int64_t n) {
    CacheLayout l{};
    const size_t rows = ((size_t)std::max<int64_t>(n, 1) * w->width * 2 + 255) & ~(size_t)255;
    l.x0 = 0, l.qs = rows, l.total = 2 * rows;
    return l;
}
extern "C" size_t foho_geo_query_cache_bytes(const foho_geo_weights* w, int64_t n_queries) {
    if (check_weights(w) != FOHO_OK || n_queries < 0) return 0;
    return cache_layout(w, n_queries).total;
}

extern "C" int foho_geo_prepare_queries(const foho_geo_weights* w, const float* queries, int64_t n_queries, int32_t chunk_rows, void* ws, size_t ws_bytes,
                                        void* cache, size_t cache_bytes, void* stream_) {
    Ws o;
    if (int rc = open_ws("foho_geo_prepare_queries", w, queries && ws && cache && chunk_rows > 0 && n_queries >= 0, chunk_rows, ws, ws_bytes, o)) return rc;
    const Layout& l = o.l;
    const CacheLayout c = cache_layout(w, n_queries);
    if (cache_bytes < c.total) return fail(FOHO_ERR_WORKSPACE, "foho_geo_prepare_queries: cache too small (foho_geo_query_cache_bytes)");
    hipStream_t s = (hipStream_t)stream_;
    char* base = o.base;
    h16 *E = (h16*)(base + l.e), *bB = (h16*)(base + l.b);
    h16 *X0 = (h16*)((char*)cache + c.x0), *Qs = (h16*)((char*)cache + c.qs);
    const size_t W = w->width;
    for (int64_t r0 = 0; r0 < n_queries; r0 += chunk_rows) {
        const int M = (int)std::min<int64_t>(chunk_rows, n_queries - r0);
        if (int rc = chain_query_side(w, queries + 3 * r0, M, E, X0 + r0 * W, bB, Qs + r0 * W, nullptr, 0, s)) return rc;
    }
    return FOHO_OK;
}

extern "C" int foho_geo_decode_fwd_cached(const foho_geo_weights* w, const float* queries, int64_t n_queries, const void* cache, size_t cache_bytes,
                                          float* logits, int32_t chunk_rows, void* ws, size_t ws_bytes, void* stream_) {
    Ws o;
    if (int rc = open_ws("foho_geo_decode_fwd_cached", w, queries && cache && logits && ws && chunk_rows > 0 && n_queries >= 0, chunk_rows, ws, ws_bytes, o)) return rc;
    const Layout& l = o.l;
    const CacheLayout c = cache_layout(w, n_queries);
    if (cache_bytes < c.total) return fail(FOHO_ERR_WORKSPACE, "foho_geo_decode_fwd_cached: cache too small");
    hipStream_t s = (hipStream_t)stream_;
    char* base = o.base;
    const h16 *kv = o.kv, *vt = o.vt;
    h16 *bA = (h16*)(base + l.a), *bB = (h16*)(base + l.b), *bC = (h16*)(base + l.c), *bH = (h16*)(base + l.h);
    const Fold fold = fold_of(w, l, base);
    const h16 *X0 = (const h16*)((const char*)cache + c.x0), *Qs = (const h16*)((const char*)cache + c.qs);
    const size_t W = w->width;
    for (int64_t r0 = 0; r0 < n_queries; r0 += chunk_rows) {
        const int M = (int)std::min<int64_t>(chunk_rows, n_queries - r0);
        // attention Qs -> B;  x1 = x0 + c_proj: B (+X0) -> C;  ln_2: C -> B;  fc1: B -> H;  x2 = x1 + fc2: H (+C) -> A
        if (int rc = chain_latent_side(w, M, X0 + r0 * W, Qs + r0 * W, bB, bC, bB, nullptr, bH, bA, nullptr, kv, vt, s, nullptr, &fold, queries + 3 * r0, logits + r0))
            return rc;
        if (!fold.w1f)
            if (int rc = chain_logits(w, queries + 3 * r0, M, bA, logits + r0, s)) return rc;
    }
    return FOHO_OK;
}

struct BwdLayout {
    size_t e, x0, xn, qs, qst, at, x1, z, h, x2, dx2, dat, lse, delta, part, total;
    int ldt, splits;
};
// workgroups of k_geo_attn_bwd per (key block, head): enough for ~4 per CU, preferring a count that fills whole rounds of the
// 512 resident workgroups (2 per CU)
static int bwd_splits(const foho_geo_weights* w, int chunk) {
    const int ntiles = (chunk + 63) / 64, base = (w->n_latents / 128) * w->heads;
    int s0 = std::max(1, (1024 + base - 1) / base), best = s0;
    double bw = 1e9;
    for (int sp = s0; sp < s0 + 4; sp++) {
        const double n = (double)base * sp, waste = std::ceil(n / 512.0) * 512.0 / n;
        if (waste < bw - 1e-9) bw = waste, best = sp;
    }
    return std::max(1, std::min(best, ntiles));
}
static BwdLayout bwd_layout(const foho_geo_weights* w, int chunk) {
    BwdLayout l{};
    Carve cv;
    const size_t W = w->width, F = w->hidden, C = chunk;
    l.ldt = (chunk + 63) & ~63;
    l.e = cv.take(C * 64 * 2);
    l.x0 = cv.take(C * W * 2);
    l.xn = cv.take(C * W * 2);
    l.qs = cv.take(C * W * 2);
    l.qst = cv.take(W * (size_t)l.ldt * 2);
    l.at = cv.take(C * W * 2);
    l.x1 = cv.take(C * W * 2);
    l.z = cv.take(C * F * 2);
    l.h = cv.take(C * F * 2);
    l.x2 = cv.take(C * W * 2);
    l.dx2 = cv.take(C * W * 2);
    l.dat = cv.take(W * (size_t)l.ldt * 2);
    l.lse = cv.take((size_t)l.ldt * w->heads * 4);    // rows up to the next multiple of 64: the padding of the last query tile
    l.delta = cv.take((size_t)l.ldt * w->heads * 4);
    l.splits = bwd_splits(w, chunk);
    l.part = cv.take((size_t)l.splits * w->n_latents * 2 * W * 4);
    l.total = cv.off;
    return l;
}

extern "C" size_t foho_geo_bwd_workspace_bytes(const foho_geo_weights* w, int32_t chunk_rows) {
    if (check_weights(w) != FOHO_OK || chunk_rows <= 0) return 0;
    return bwd_layout(w, chunk_rows).total;
}

extern "C" int foho_geo_set_kv(const foho_geo_weights* w, const void* kv_in, int32_t chunk_rows, void* ws, size_t ws_bytes, void* stream_) {
    Ws o;
    if (int rc = open_ws("foho_geo_set_kv", w, kv_in && ws && chunk_rows > 0, chunk_rows, ws, ws_bytes, o)) return rc;
    hipStream_t s = (hipStream_t)stream_;
    if (hipMemcpyAsync(o.kv, kv_in, (size_t)w->n_latents * 2 * w->width * 2, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(FOHO_ERR_LAUNCH, "foho_geo_set_kv: copy failed");
    return finish_kv(w, o, s);
}

// What the backward of one row block needs from its forward: per block in the `save` buffer (kept mode) or in the backward
// workspace (recompute mode)
struct SavedLayout {
    size_t qs, qst, at, x1, z, x2, lse, total;
};
static SavedLayout saved_layout(const foho_geo_weights* w, int chunk) {
    SavedLayout l{};
    Carve cv;
    const size_t W = w->width, F = w->hidden, C = chunk, ldt = (chunk + 63) & ~63;
    l.qs = cv.take(C * W * 2);
    l.qst = cv.take(W * ldt * 2);
    l.at = cv.take(C * W * 2);
    l.x1 = cv.take(C * W * 2);
    l.z = cv.take(C * F * 2);
    l.x2 = cv.take(C * W * 2);
    l.lse = cv.take(ldt * (size_t)w->heads * 4);
    l.total = cv.off;
    return l;
}
struct ChunkPtrs {
    h16 *E, *X0, *Xn, *H, *dX2, *dAT;        // scratch
    h16 *Qs, *QsT, *At, *X1, *Z, *X2;        // saved by the forward
    float *lse, *delta;
    int ldt;
};

// the forward chain of one row block with everything its backward needs kept (P.Qs .. P.lse)
static int chain_fwd_keep(const foho_geo_weights* w, const float* q, int M, const ChunkPtrs& P, const h16* kv, const h16* vt, hipStream_t s,
                          const int* Mdev = nullptr) {
    if (int rc = chain_query_side(w, q, M, P.E, P.X0, P.Xn, P.Qs, P.QsT, P.ldt, s, Mdev)) return rc;
    return chain_latent_side(w, M, P.X0, P.Qs, P.At, P.X1, P.Xn, P.Z, P.H, P.X2, P.lse, kv, vt, s, Mdev);
}

// ... and backwards: logits -> ln_post -> fc2 -> GELU -> fc1 -> ln_2 (+ residual) -> c_proj -> attention (K, V partial sums)
static int chain_bwd(const foho_geo_weights* w, const float* grad_logits, int M, const ChunkPtrs& P, const h16* kv, int splits, int accumulate, float* part,
                     hipStream_t s, const int* Mdev = nullptr) {
    const int W = w->width, Lr = w->n_latents, F = w->hidden, NH = w->heads;
    ln_logits_bwd(s, w, P.X2, grad_logits, P.dX2, M, Mdev);
    if (int rc = gemm(dense(P.dX2, w->w_fc2_t, P.H, M, F, W, Mdev), Epi(w->zeros).gelu_bwd(P.Z, F), s)) return rc;     // dZ -> H
    if (int rc = gemm(dense(P.H, w->w_fc1_t, P.Xn, M, W, F, Mdev), Epi(w->zeros), s)) return rc;                       // d ln_2 out -> Xn
    ln_rows_bwd(s, P.X1, w->ln_2_g, eps_of(w, w->ln_2_eps), P.Xn, P.dX2, P.X0, M, W, Mdev);                            // dX1 -> X0
    if (int rc = gemm(dense(P.X0, w->w_proj_t, P.dX2, M, W, W, Mdev), Epi(w->zeros).trans(P.dAT, P.ldt), s)) return rc;   // dO -> dX2
    delta(s, P.dX2, P.At, W, NH, M, P.delta, Mdev);
    if (!launch_ok("geometry decoder backward chain (row kernels)")) return FOHO_ERR_LAUNCH;
    AttnBwd b;
    b.Qs = P.Qs, b.QsT = P.QsT, b.dO = P.dX2, b.dOT = P.dAT, b.ldt = P.ldt, b.nlse = P.lse, b.ndelta = P.delta, b.KV = kv, b.ldkv = 2 * W, b.width = W, b.heads = NH;
    b.M = M, b.L = Lr, b.splits = splits, b.accumulate = accumulate, b.part = part, b.Mdev = Mdev;
    attn_bwd(s, b);
    return launch_ok("k_geo_attn_bwd") ? FOHO_OK : FOHO_ERR_LAUNCH;
}

static ChunkPtrs chunk_ptrs(const BwdLayout& b, char* base, const SavedLayout& sl, char* saved) {
    ChunkPtrs P;
    P.E = (h16*)(base + b.e), P.X0 = (h16*)(base + b.x0), P.Xn = (h16*)(base + b.xn), P.H = (h16*)(base + b.h), P.dX2 = (h16*)(base + b.dx2);
    P.dAT = (h16*)(base + b.dat), P.delta = (float*)(base + b.delta), P.ldt = b.ldt;
    if (saved) {
        P.Qs = (h16*)(saved + sl.qs), P.QsT = (h16*)(saved + sl.qst), P.At = (h16*)(saved + sl.at), P.X1 = (h16*)(saved + sl.x1);
        P.Z = (h16*)(saved + sl.z), P.X2 = (h16*)(saved + sl.x2), P.lse = (float*)(saved + sl.lse);
    } else {
        P.Qs = (h16*)(base + b.qs), P.QsT = (h16*)(base + b.qst), P.At = (h16*)(base + b.at), P.X1 = (h16*)(base + b.x1);
        P.Z = (h16*)(base + b.z), P.X2 = (h16*)(base + b.x2), P.lse = (float*)(base + b.lse);
    }
    return P;
}

extern "C" size_t foho_geo_saved_bytes(const foho_geo_weights* w, int32_t chunk_rows, int64_t n_queries) {
    if (check_weights(w) != FOHO_OK || chunk_rows <= 0 || n_queries < 0) return 0;
    const int64_t nchunks = (n_queries + chunk_rows - 1) / chunk_rows;
    return (size_t)std::max<int64_t>(nchunks, 1) * saved_layout(w, chunk_rows).total;
}

static int bwd_args(const char* who, const foho_geo_weights* w, const void* a, const void* b_, const void* ws, const void* bws, int32_t chunk_rows,
                    int64_t n_queries, bool need_t) {
    if (int rc = check_weights(w)) return rc;
    if (!a || !b_ || !ws || !bws || chunk_rows <= 0 || n_queries < 0) return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": null argument");
    if (need_t && (!w->w_fc2_t || !w->w_fc1_t || !w->w_proj_t || !w->zeros)) return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": transposed weights / zeros missing");
    if (w->n_latents % 128) return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": n_latents must be a multiple of 128");
    return FOHO_OK;
}

extern "C" int foho_geo_decode_fwd_keep(const foho_geo_weights* w, const float* queries, int64_t n_queries, float* logits, int32_t chunk_rows, void* ws,
                                        size_t ws_bytes, void* bws, size_t bws_bytes, void* saved, size_t saved_bytes, void* stream_) {
    if (int rc = bwd_args("foho_geo_decode_fwd_keep", w, queries, logits, ws, bws, chunk_rows, n_queries, false)) return rc;
    const Ws o = ws_of(w, chunk_rows, ws);
    const BwdLayout b = bwd_layout(w, chunk_rows);
    const SavedLayout sl = saved_layout(w, chunk_rows);
    if (ws_bytes < o.l.total || bws_bytes < b.total) return fail(FOHO_ERR_WORKSPACE, "foho_geo_decode_fwd_keep: workspace too small");
    if (!saved || saved_bytes < foho_geo_saved_bytes(w, chunk_rows, n_queries)) return fail(FOHO_ERR_WORKSPACE, "foho_geo_decode_fwd_keep: buffer for the activations too small");
    hipStream_t s = (hipStream_t)stream_;
    const h16 *kv = o.kv, *vt = o.vt;
    for (int64_t r0 = 0, c = 0; r0 < n_queries; r0 += chunk_rows, c++) {
        const int M = (int)std::min<int64_t>(chunk_rows, n_queries - r0);
        const ChunkPtrs P = chunk_ptrs(b, (char*)bws, sl, (char*)saved + c * sl.total);
        // columns of Qs^T beyond a ragged block's rows meet P = 0 in the backward and must be finite
        if ((M & 63) && hipMemsetAsync(P.QsT, 0, (size_t)w->width * b.ldt * 2, s) != hipSuccess) return fail(FOHO_ERR_LAUNCH, "foho_geo_decode_fwd_keep: memset failed");
        if (int rc = chain_fwd_keep(w, queries + 3 * r0, M, P, kv, vt, s)) return rc;
        if (int rc = chain_logits(w, queries + 3 * r0, M, P.X2, logits + r0, s)) return rc;
    }
    return FOHO_OK;
}

extern "C" int foho_geo_decode_bwd(const foho_geo_weights* w, const float* queries, int64_t n_queries, const float* grad_logits, float* grad_kv,
                                   int32_t chunk_rows, void* ws, size_t ws_bytes, void* bws, size_t bws_bytes, const void* saved, size_t saved_bytes,
                                   void* stream_) {
    if (int rc = bwd_args("foho_geo_decode_bwd", w, queries, grad_logits, ws, bws, chunk_rows, n_queries, true)) return rc;
    if (!grad_kv) return fail(FOHO_ERR_BAD_ARG, "foho_geo_decode_bwd: null argument");
    const Ws o = ws_of(w, chunk_rows, ws);
    const BwdLayout b = bwd_layout(w, chunk_rows);
    const SavedLayout sl = saved_layout(w, chunk_rows);
    if (ws_bytes < o.l.total || bws_bytes < b.total) return fail(FOHO_ERR_WORKSPACE, "foho_geo_decode_bwd: workspace too small");
    if (saved && saved_bytes < foho_geo_saved_bytes(w, chunk_rows, n_queries)) return fail(FOHO_ERR_WORKSPACE, "foho_geo_decode_bwd: buffer of activations too small");
    hipStream_t s = (hipStream_t)stream_;
    const h16 *kv = o.kv, *vt = o.vt;
    char* base = (char*)bws;
    const int W = w->width, Lr = w->n_latents;
    // columns of the transposed copies beyond a ragged block's rows must be finite (they meet P = 0): clear them once
    if (hipMemsetAsync(base + b.dat, 0, (size_t)W * b.ldt * 2, s) != hipSuccess || (!saved && hipMemsetAsync(base + b.qst, 0, (size_t)W * b.ldt * 2, s) != hipSuccess))
        return fail(FOHO_ERR_LAUNCH, "foho_geo_decode_bwd: memset failed");
    float* part = (float*)(base + b.part);
    if (n_queries == 0) return hipMemsetAsync(grad_kv, 0, (size_t)Lr * 2 * W * 4, s) == hipSuccess ? FOHO_OK : fail(FOHO_ERR_LAUNCH, "foho_geo_decode_bwd: memset failed");
    for (int64_t r0 = 0, c = 0; r0 < n_queries; r0 += chunk_rows, c++) {
        const int M = (int)std::min<int64_t>(chunk_rows, n_queries - r0);
        const ChunkPtrs P = chunk_ptrs(b, base, sl, saved ? (char*)const_cast<void*>(saved) + c * sl.total : nullptr);
        if (!saved)
            if (int rc = chain_fwd_keep(w, queries + 3 * r0, M, P, kv, vt, s)) return rc;
        if (int rc = chain_bwd(w, grad_logits + r0, M, P, kv, b.splits, r0 > 0 ? 1 : 0, part, s)) return rc;
    }
    return dkv_reduce(s, part, b.splits, Lr, W, grad_kv);
}

// ---- backward over the ACTIVE rows only.  The gradient that reaches latent2sdf comes out of FlexiCubes (PL:1507-1509, 1600): it is
// non-zero on the end points of the grid edges the iso-surface crosses -- 5-10 % of the 65^3 rows.  A row whose logit gradient is zero
// contributes exactly zero to dK / dV, so the rows with grad_logits != 0 are compacted ON THE DEVICE (in row order: deterministic),
// the forward chain is recomputed for them and the backward runs on them.  The count stays in device memory: every launch is sized
// for a row block of the capacity and works on min(block, what is left of the count) rows -- blocks beyond the count leave at once --
// so there is no host synchronisation and the call can be captured in a hipGraph.
struct RowsLayout {
    size_t counts, mblk, q, g, idx, total;
    int nscan, nblk;
};
constexpr int ROWS_PER_WG = 2048;
static RowsLayout rows_layout(int64_t n, int64_t cap, int chunk) {
    RowsLayout l{};
    Carve cv;
    l.nscan = (int)((n + ROWS_PER_WG - 1) / ROWS_PER_WG);
    l.nblk = (int)std::max<int64_t>((cap + chunk - 1) / chunk, 1);
    l.counts = cv.take((size_t)std::max(l.nscan, 1) * 4);
    l.mblk = cv.take((size_t)(std::max(l.nblk, 1) + 2) * 4);     // [0]: the count, [1]: rows dropped for lack of capacity, [2 + c]: rows of block c
    l.q = cv.take((size_t)std::max<int64_t>(cap, 1) * 12);
    l.g = cv.take((size_t)std::max<int64_t>(cap, 1) * 4);
    l.idx = cv.take((size_t)std::max<int64_t>(cap, 1) * 4);
    l.total = cv.off;
    return l;
}

extern "C" size_t foho_geo_rows_workspace_bytes(int64_t n_queries, int64_t row_cap, int32_t chunk_rows) {
    if (n_queries < 0 || chunk_rows <= 0) return 0;
    if (row_cap <= 0 || row_cap > n_queries) row_cap = n_queries;
    return rows_layout(n_queries, row_cap, chunk_rows).total;
}

extern "C" int foho_geo_decode_bwd_rows(const foho_geo_weights* w, const float* queries, int64_t n_queries, const float* grad_logits, float* grad_kv,
                                        int64_t row_cap, int32_t chunk_rows, void* ws, size_t ws_bytes, void* bws, size_t bws_bytes, void* rows_ws,
                                        size_t rows_ws_bytes, int32_t* stats_out, void* stream_) {
    if (int rc = bwd_args("foho_geo_decode_bwd_rows", w, queries, grad_logits, ws, bws, chunk_rows, n_queries, true)) return rc;
    if (!grad_kv || !rows_ws) return fail(FOHO_ERR_BAD_ARG, "foho_geo_decode_bwd_rows: null argument");
    if (n_queries >= ((int64_t)1 << 31)) return fail(FOHO_ERR_BAD_ARG, "foho_geo_decode_bwd_rows: row indices are 32-bit");
    if (row_cap <= 0 || row_cap > n_queries) row_cap = n_queries;
    const Ws o = ws_of(w, chunk_rows, ws);
    const BwdLayout b = bwd_layout(w, chunk_rows);
    const SavedLayout sl = saved_layout(w, chunk_rows);
    const RowsLayout rl = rows_layout(n_queries, row_cap, chunk_rows);
    if (ws_bytes < o.l.total || bws_bytes < b.total || rows_ws_bytes < rl.total) return fail(FOHO_ERR_WORKSPACE, "foho_geo_decode_bwd_rows: workspace too small");
    hipStream_t s = (hipStream_t)stream_;
    const h16 *kv = o.kv, *vt = o.vt;
    char *base = (char*)bws, *rb = (char*)rows_ws;
    const int W = w->width, Lr = w->n_latents;
    int *counts = (int*)(rb + rl.counts), *mblk = (int*)(rb + rl.mblk), *idx = (int*)(rb + rl.idx);
    float *qa = (float*)(rb + rl.q), *ga = (float*)(rb + rl.g);
    // the transposed copies' columns beyond a ragged block's rows must be finite (they meet P = 0): cleared by a kernel, not a memset (zero16)
    zero16(s, (h16*)(base + b.dat), (size_t)W * b.ldt);
    zero16(s, (h16*)(base + b.qst), (size_t)W * b.ldt);
    // one workgroup per segment of ROWS_PER_WG rows, in both kernels
    hipLaunchKernelGGL(k_geo_rows_count, dim3(std::max(rl.nscan, 1)), dim3(256), 0, s, grad_logits, n_queries, counts);
    hipLaunchKernelGGL(k_geo_rows_compact, dim3(std::max(rl.nscan, 1)), dim3(256), 0, s, grad_logits, queries, n_queries, counts, rl.nscan, row_cap, chunk_rows, rl.nblk,
                       mblk, qa, ga, idx, stats_out);
    if (!launch_ok("k_geo_rows_compact")) return FOHO_ERR_LAUNCH;
    float* part = (float*)(base + b.part);
    const ChunkPtrs P = chunk_ptrs(b, base, sl, nullptr);
    for (int64_t r0 = 0, c = 0; c < std::max(rl.nblk, 1); r0 += chunk_rows, c++) {
        const int M = (int)std::max<int64_t>(std::min<int64_t>(chunk_rows, row_cap - r0), 1);
        const int* Mdev = mblk + 2 + c;
        if (int rc = chain_fwd_keep(w, qa + 3 * r0, M, P, kv, vt, s, Mdev)) return rc;
        if (int rc = chain_bwd(w, ga + r0, M, P, kv, b.splits, c > 0 ? 1 : 0, part, s, Mdev)) return rc;
    }
    return dkv_reduce(s, part, b.splits, Lr, W, grad_kv);
}

// ---- Attention as an operator of its own, forward and backward (round 5): O = softmax(Q K^T / 8) V per head of 64, what
// torch.nn.functional.scaled_dot_product_attention computes for the self-attention layers of the ShapeVAE transformer that latent2sdf
// runs in front of the decoder (PL:295; sixteen layers of 3072 tokens x 16 heads, forward and backward in every inner iteration).
// The forward is the decoder's k_geo_attn, dK / dV its k_geo_attn_bwd, dQ k_geo_attn_dq.
struct SdpaLayout {
    size_t vt, kt, qs, qst, dot, delta, part, total;
    int ldt, splits;
};
static SdpaLayout sdpa_layout(int M, int L, int heads) {
    SdpaLayout l{};
    Carve cv;
    const size_t W = (size_t)heads * 64;
    l.ldt = (M + 63) & ~63;
    l.vt = cv.take(W * L * 2);
    l.kt = cv.take(W * L * 2);
    l.qs = cv.take(W * (size_t)M * 2);
    l.qst = cv.take(W * (size_t)l.ldt * 2);
    l.dot = cv.take(W * (size_t)l.ldt * 2);
    l.delta = cv.take((size_t)l.ldt * heads * 4);
    const int ntiles = (M + 63) / 64, base = std::max(1, (L / 128) * heads);
    l.splits = std::max(1, std::min((1024 + base - 1) / base, ntiles));
    l.part = cv.take((size_t)l.splits * L * 2 * W * 4);
    l.total = cv.off;
    return l;
}
static int sdpa_args(const char* who, const foho_sdpa_desc* d, bool bwd) {
    if (!d) return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": null descriptor");
    const int M = d->M, L = d->L, heads = d->heads;
    if (M < 1 || L < 64 || L % 64 || heads < 1 || heads > 16 || d->batch < 1)
        return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": M >= 1, L a multiple of 64, 1..16 heads of 64, batch >= 1");
    if (bwd && L % 128) return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": L must be a multiple of 128");
    if (d->q_row < 64 || d->kv_row < 64 || d->q_head < 64 || d->kv_head < 64 || (d->q_row & 7) || (d->kv_row & 7) || (d->q_head & 7) || (d->kv_head & 7) ||
        (d->q_batch & 7) || (d->kv_batch & 7))
        return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": strides must be multiples of 8 halfs (16-byte rows), at least 64");
    if (((size_t)(L - 1) * d->kv_row + (size_t)(heads - 1) * d->kv_head + 64) * 2 >= ((size_t)1 << 31) ||
        ((size_t)(M - 1) * d->q_row + (size_t)(heads - 1) * d->q_head + 64) * 2 >= ((size_t)1 << 31))
        return fail(FOHO_ERR_BAD_ARG, std::string(who) + ": operand too large for 32-bit buffer offsets");
    return FOHO_OK;
}

extern "C" size_t foho_sdpa_workspace_bytes(int32_t M, int32_t L, int32_t heads) {
    foho_sdpa_desc d{};
    d.M = M, d.L = L, d.heads = heads, d.batch = 1, d.q_row = d.kv_row = heads * 64, d.q_head = d.kv_head = 64;
    if (sdpa_args("foho_sdpa_workspace_bytes", &d, false) != FOHO_OK) return 0;
    return sdpa_layout(M, L, heads).total;
}
extern "C" int foho_sdpa_fwd(const foho_sdpa_desc* d, const void* q, const void* k, const void* v, void* out, float* nlse, float* lse_nat, void* ws,
                             size_t ws_bytes, void* stream_) {
    if (int rc = sdpa_args("foho_sdpa_fwd", d, false)) return rc;
    if (!q || !k || !v || !out || !ws) return fail(FOHO_ERR_BAD_ARG, "foho_sdpa_fwd: null argument");
    const int M = d->M, L = d->L, heads = d->heads, W = heads * 64;
    const SdpaLayout l = sdpa_layout(M, L, heads);
    if (ws_bytes < l.total) return fail(FOHO_ERR_WORKSPACE, "foho_sdpa_fwd: workspace too small");
    hipStream_t s = (hipStream_t)stream_;
    h16* vt = (h16*)((char*)ws + l.vt);
    const size_t nl = (size_t)((M + 63) & ~63) * heads;
    AttnFwd a;
    a.ldq = (int)d->q_row, a.qhs = (int)d->q_head, a.ldk = (int)d->kv_row, a.khs = (int)d->kv_head, a.Vt = vt, a.L = L, a.ldo = W, a.M = M, a.heads = heads, a.qscale = QSCALE;
    for (int b = 0; b < d->batch; b++) {
        const h16* vb = (const h16*)v + (size_t)b * d->kv_batch;
        a.Q = (const h16*)q + (size_t)b * d->q_batch, a.K = (const h16*)k + (size_t)b * d->kv_batch, a.O = (h16*)out + (size_t)b * M * W;
        a.nlse = nlse ? nlse + b * nl : nullptr, a.lse_nat = lse_nat ? lse_nat + (size_t)b * heads * M : nullptr;
        pack_vt(s, vb, (int)d->kv_row, W, L, vt, 0, (int)d->kv_head);
        attn_fwd(s, a);
    }
    return launch_ok("k_geo_attn") ? FOHO_OK : FOHO_ERR_LAUNCH;
}
// The backward of one image: dQ, dK, dV from q / k / v where they lie, the forward's output and -lse, and dO (M, 64 heads; contiguous rows).
// gq rows have stride ldgq, gk / gv rows ldgkv (heads side by side in all three).
static int sdpa_bwd_image(const SdpaLayout& l, char* base, const h16* qb, int q_row, int q_head, const h16* kb, const h16* vb, int kvr, int kvh, const h16* O,
                          const h16* dO, const float* nls, h16* gq, int ldgq, h16* gk, h16* gv, int ldgkv, int M, int L, int heads, hipStream_t s) {
    const int W = heads * 64;
    h16 *kt = (h16*)(base + l.kt), *qs = (h16*)(base + l.qs), *qst = (h16*)(base + l.qst), *dot = (h16*)(base + l.dot);
    float *ndelta = (float*)(base + l.delta), *part = (float*)(base + l.part);
    pack_vt(s, kb, kvr, W, L, kt, 0, kvh);      // K^T, key-permuted
    if (M & 63) {   // columns of the transposed copies beyond M meet P = 0 and must be finite
        zero16(s, qst, (size_t)W * l.ldt);
        zero16(s, dot, (size_t)W * l.ldt);
    }
    transpose_perm(s, qb, q_row, M, W, qst, l.ldt, q_head, QSCALE, qs);
    transpose_perm(s, dO, W, M, W, dot, l.ldt);
    delta(s, dO, O, W, heads, M, ndelta);
    if (!launch_ok("sdpa backward (row kernels)")) return FOHO_ERR_LAUNCH;
    AttnBwd b;
    b.Qs = qs, b.QsT = qst, b.dO = dO, b.dOT = dot, b.ldt = l.ldt, b.nlse = nls, b.ndelta = ndelta, b.KV = kb, b.Vp = vb, b.ldkv = kvr, b.khs = kvh, b.width = W, b.heads = heads;
    b.M = M, b.L = L, b.dk16 = gk, b.dv16 = gv, b.ld16 = ldgkv;
    AttnDq g;
    g.Qs = qs, g.dO = dO, g.ldq = W, g.KV = kb, g.Vp = vb, g.ldkv = kvr, g.khs = kvh, g.width = W, g.Kt = kt, g.L = L, g.nlse = nls, g.ndelta = ndelta, g.dQ = gq, g.lddq = ldgq;
    g.M = M, g.heads = heads;
    // enough (head, key block) workgroups to fill the chip on their own: each walks ALL query tiles and writes its dK / dV itself (no
    // partial sums, no reduction pass: -14 us at 16 heads x 3072 keys); otherwise splits of the query tiles + k_geo_dkv_reduce16
    if ((long)heads * (L / 128) < 256) return attn_bwd_split(s, b, g, l.splits, part);
    b.part = part;   // (not written on the direct route)
    attn_bwd(s, b);
    attn_dq(s, g);
    return launch_ok("k_geo_attn_dq") ? FOHO_OK : FOHO_ERR_LAUNCH;
}
extern "C" int foho_sdpa_bwd(const foho_sdpa_desc* d, const void* q, const void* k, const void* v, const void* out, const float* nlse, const void* grad_out,
                             void* grad_q, void* grad_k, void* grad_v, void* ws, size_t ws_bytes, void* stream_) {
    if (int rc = sdpa_args("foho_sdpa_bwd", d, true)) return rc;
    if (!q || !k || !v || !out || !nlse || !grad_out || !grad_q || !grad_k || !grad_v || !ws) return fail(FOHO_ERR_BAD_ARG, "foho_sdpa_bwd: null argument");
    const int M = d->M, L = d->L, heads = d->heads, W = heads * 64;
    const SdpaLayout l = sdpa_layout(M, L, heads);
    if (ws_bytes < l.total) return fail(FOHO_ERR_WORKSPACE, "foho_sdpa_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream_;
    const size_t nl = (size_t)((M + 63) & ~63) * heads;
    for (int b = 0; b < d->batch; b++) {
        const h16 *qb = (const h16*)q + (size_t)b * d->q_batch, *kb = (const h16*)k + (size_t)b * d->kv_batch, *vb = (const h16*)v + (size_t)b * d->kv_batch;
        if (int rc = sdpa_bwd_image(l, (char*)ws, qb, (int)d->q_row, (int)d->q_head, kb, vb, (int)d->kv_row, (int)d->kv_head, (const h16*)out + (size_t)b * M * W,
                                    (const h16*)grad_out + (size_t)b * M * W, nlse + b * nl, (h16*)grad_q + (size_t)b * M * W, W, (h16*)grad_k + (size_t)b * L * W,
                                    (h16*)grad_v + (size_t)b * L * W, W, M, L, heads, s))
            return rc;
    }
    return FOHO_OK;
}

// Unit entry points (tests / profiling): the GEMM and the attention kernel on their own.
extern "C" int foho_geo_gemm(const void* A, const void* Wt, const float* bias, const void* R, void* C, int32_t M, int32_t N, int32_t K,
                             int32_t gelu, float scale, void* stream) {
    if (!A || !Wt || !bias || !C) return fail(FOHO_ERR_BAD_ARG, "foho_geo_gemm: null argument");
    if ((gelu & 1) && R) return fail(FOHO_ERR_BAD_ARG, "foho_geo_gemm: GELU and a residual are not combined on this path");
    Gemm g = dense((const h16*)A, Wt, (h16*)C, M, N, K);
    g.scale = scale;
    g.variant = (gelu & 2) ? GV_128 : (gelu & 4) ? GV_LOCKSTEP : (gelu & 8) ? GV_DEEP : (gelu & 16) ? GV_PHASED : (gelu & 32) ? GV_PC : (gelu & 64) ? GV_PHASED192 : GV_AUTO;
    Epi e(bias);
    if (gelu & 1) e.gelu();
    else if (R) e.resid((const h16*)R, N);
    return gemm(g, e, (hipStream_t)stream);
}

extern "C" int foho_geo_attention(const void* Q, const void* KV, void* Vt_scratch, void* O, int32_t M, int32_t n_latents, int32_t heads,
                                  void* stream) {
    if (!Q || !KV || !Vt_scratch || !O || heads <= 0 || n_latents <= 0 || n_latents % 64 || (size_t)n_latents * heads * 256 >= ((size_t)1 << 31))
        return fail(FOHO_ERR_BAD_ARG, "foho_geo_attention: bad argument");
    const int W = heads * 64;
    hipStream_t s = (hipStream_t)stream;
    pack_vt(s, (const h16*)KV, 2 * W, W, n_latents, (h16*)Vt_scratch);
    if (!launch_ok("k_geo_pack_vt")) return FOHO_ERR_LAUNCH;
    if (M <= 0) return FOHO_OK;
    AttnFwd a;
    a.Q = (const h16*)Q, a.ldq = W, a.K = (const h16*)KV, a.ldk = 2 * W, a.Vt = (const h16*)Vt_scratch, a.L = n_latents, a.O = (h16*)O, a.ldo = W, a.M = M, a.heads = heads;
    attn_fwd(s, a);
    return launch_ok("k_geo_attn") ? FOHO_OK : FOHO_ERR_LAUNCH;
}
