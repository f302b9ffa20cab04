// rastk_blend.inc -- foho_rastk_blend_fwd / _bwd (foho_rastk.h): interpolate_face_attributes + softmax_rgb_blend over the K planes
// foho_rastk_fwd writes, one launch each way.  Included by foho_rastk.hip behind its entry points (fail / launched / blocks_for / TPB
// are foho_side.h's).  DESIGN.md section 3C.
//
// One thread per pixel, no LDS, no workspace.  The sweeps are templates over where a pixel's fragments come from and where their
// gradients go, so that rastk_render.inc runs the same arithmetic on the keys k_rk_select keeps in LDS.  The planes are front-packed: a pixel's fragments are its n leading entries with an id
// in 0 .. F-1, and every sweep stops at n, so a pixel costs what it holds, not K.  Nothing K-sized lives in registers: what a later
// sweep needs of an earlier one it recomputes from the planes.
//   forward   sweep A: n, max_k zinv_k and its first index; sweep B: p, q = 1 - p, w, the sums S = sum w, num_c = sum w c_kc, the
//             product of the q (as a count of exact zeros and the product of the others)
//   backward  sweeps A and B again, then sweep C: the gradients of fragment k from the pixel's sums
// Every sum runs over k = 0 .. n-1 in that order in one thread: out and the three plane gradients are bitwise repeatable.  Only
// grad_face_attr is added with float atomics.
namespace {

constexpr float BLEND_EPS = 1e-10f;  // softmax_rgb_blend's eps

struct BlendCfg {
    float sigma, gamma, zfar, zrange;  // zrange = zfar - znear
    float bg[4];
    int K;
    int64_t F;  // ids outside 0 .. F-1 end a pixel's prefix (alpha only: ids < 0)
    size_t pixels;
};

// p = sigmoid(-d / sigma) and q = 1 - p, each from the side of the exponential that cannot overflow and without the cancellation of
// 1 - p: t = exp(-|x|) <= 1.  |x| = 1e6 gives t = 0 and (p, q) = (1, 0) or (0, 1) exactly.
__device__ __forceinline__ void sigmoid_pq(float d, float sigma, float& p, float& q) {
    const float x = -d / sigma;
    const float t = expf(-fabsf(x));
    const float a = 1.0f / (1.0f + t), b = t / (1.0f + t);
    p = x >= 0.0f ? a : b;
    q = x >= 0.0f ? b : a;
}

// the product of the q_k as (number of exact zeros, product of the others): the exclusive product over j != k is then
// pnz / q_k with no zero, pnz for the one zero factor, and 0 otherwise -- never full product / q_k
struct QProd {
    float pnz;
    int nzero;
    __device__ __forceinline__ void mul(float q) {
        if (q == 0.0f) nzero++;
        else pnz *= q;
    }
    __device__ __forceinline__ float full() const { return nzero ? 0.0f : pnz; }
    __device__ __forceinline__ float without(float q) const { return nzero == 0 ? pnz / q : (nzero == 1 && q == 0.0f ? pnz : 0.0f); }
};

// c_kc = sum_j bary_kj attr[face, j, c], j ascending (UNIT: weights 1, bary is not read)
template <int D, bool UNIT>
__device__ __forceinline__ void frag_colour(const float* __restrict__ fa, const float* __restrict__ b, float* col) {
#pragma unroll
    for (int c = 0; c < D; c++) col[c] = UNIT ? (fa[c] + fa[D + c]) + fa[2 * D + c] : (b[0] * fa[c] + b[1] * fa[D + c]) + b[2] * fa[2 * D + c];
}

template <int D>
struct PixSums {
    int n, amax;        // fragments of the pixel; first index of the largest zinv
    float m;            // max(max_k zinv_k, eps)
    bool m_passes;      // the max was not clamped: its gradient reaches fragment amax
    float draw, delta;  // exp((eps - m) / gamma) and its clamp at eps
    float S, num[D];    // sum_k w_k, sum_k w_k c_kc
    QProd q;
};

__device__ __forceinline__ float zinv_of(float z, const BlendCfg& c) { return (c.zfar - z) / c.zrange; }

// A pixel's fragments as the sweeps see them -- has(k): k is one of them (they are the leading k); z(k), face(k); shade<BARY>(k, d, b):
// the distance and, with BARY, the three barycentrics.  PlaneFrags reads the K planes; SlabFrags (rastk_render.inc) the sorted keys of
// k_rk_select's slab.  The sweeps below are the one copy of the blend's arithmetic for both.
struct PlaneFrags {
    const int64_t* id;
    const float *zb, *ba, *di;
    int K;
    int64_t lim;  // ids outside 0 .. lim-1 end the pixel's fragments
    __device__ __forceinline__ bool has(int k) const { return k < K && id[k] >= 0 && id[k] < lim; }
    __device__ __forceinline__ float z(int k) const { return zb[k]; }
    __device__ __forceinline__ int64_t face(int k) const { return id[k]; }
    template <bool BARY>
    __device__ __forceinline__ void shade(int k, float& d, float* b) const {
        d = di[k];
        if (BARY) b[0] = ba[3 * k], b[1] = ba[3 * k + 1], b[2] = ba[3 * k + 2];
    }
};

// where sweep C's per-fragment gradients go: PlaneSink writes them into the plane gradients (each may be NULL)
struct PlaneSink {
    float *g_z, *g_b, *g_d;
    __device__ __forceinline__ void emit(int k, int64_t, float gz, const float* gb, float gd) const {
        if (g_z) g_z[k] = gz;
        if (g_d) g_d[k] = gd;
        if (g_b) g_b[3 * k] = gb[0], g_b[3 * k + 1] = gb[1], g_b[3 * k + 2] = gb[2];
    }
};

// sweeps A and B of one pixel
template <int D, bool UNIT, class FRAGS>
__device__ __forceinline__ PixSums<D> pixel_sums(const FRAGS& fr, const float* __restrict__ attr, const BlendCfg& c) {
    PixSums<D> s;
    s.n = 0, s.amax = 0;
    float zmax = 0.0f;
    for (int k = 0; fr.has(k); k++) {
        const float zi = zinv_of(fr.z(k), c);
        if (k == 0 || zi > zmax) zmax = zi, s.amax = k;
        s.n = k + 1;
    }
    s.m_passes = s.n > 0 && zmax >= BLEND_EPS;
    s.m = s.m_passes ? zmax : BLEND_EPS;
    s.draw = expf((BLEND_EPS - s.m) / c.gamma);
    s.delta = fmaxf(s.draw, BLEND_EPS);
    s.S = 0.0f;
#pragma unroll
    for (int ch = 0; ch < D; ch++) s.num[ch] = 0.0f;
    s.q.pnz = 1.0f, s.q.nzero = 0;
    for (int k = 0; k < s.n; k++) {
        float p, q, col[D], d, b[3];
        fr.template shade<!UNIT>(k, d, b);
        sigmoid_pq(d, c.sigma, p, q);
        s.q.mul(q);
        const float w = p * expf((zinv_of(fr.z(k), c) - s.m) / c.gamma);
        frag_colour<D, UNIT>(attr + (size_t)fr.face(k) * 3 * D, b, col);
        s.S += w;
#pragma unroll
        for (int ch = 0; ch < D; ch++) s.num[ch] += w * col[ch];
    }
    return s;
}

// the pixel of the image from its sums: the D blended channels, then alpha
template <int D>
__device__ __forceinline__ void write_pixel(const PixSums<D>& s, const BlendCfg& c, float* po) {
    const float den = s.S + s.delta;
#pragma unroll
    for (int ch = 0; ch < D; ch++) po[ch] = (s.num[ch] + s.delta * c.bg[ch]) / den;  // no fragment: (0 + 1 bg) / 1
    po[D] = 1.0f - s.q.full();
}

// sweep C of one pixel with fragments: the gradients of fragment k from the pixel's sums, to the sink (g_bary is 0 with UNIT), and the
// attribute gradient by float atomicAdd (g_attr may be NULL).  go: the pixel's D + 1 entries of grad_out.
template <int D, bool UNIT, class FRAGS, class SINK>
__device__ __forceinline__ void pixel_grads(const FRAGS& fr, const PixSums<D>& s, const float* __restrict__ attr, const BlendCfg& c,
                                            const float* __restrict__ go, const SINK& sink, float* g_attr) {
    const float den = s.S + s.delta;
    // rgb_c = (num_c + delta bg_c) / den: gn_c = dL/dnum_c; dL/dw_k = sum_c gn_c (c_kc - rgb_c); dL/ddelta = sum_c gn_c (bg_c - rgb_c)
    float gn[D], rgb[D], g_delta = 0.0f;
#pragma unroll
    for (int ch = 0; ch < D; ch++) {
        rgb[ch] = (s.num[ch] + s.delta * c.bg[ch]) / den;
        gn[ch] = go[ch] / den;
        g_delta += gn[ch] * (c.bg[ch] - rgb[ch]);
    }
    const float g_alpha = go[D];  // out alpha = 1 - prod q: d alpha / d p_k = prod_{j != k} q_j
    // m enters every exponent and, where delta is not clamped, delta.  With u_k = dL/d(zinv_k - m) = dL/dw_k w_k / gamma the max's
    // gradient is -(sum_k u_k + v), v = dL/ddelta delta / gamma where delta is not clamped and 0 where it is, and torch sends it to
    // fragment amax, whose own u cancels: it receives -(sum_{k != amax} u_k + v), summed WITHOUT that term.  So a pixel's only
    // fragment gets exactly -v (0 where delta is clamped, as in torch), and the nearest fragment, whose colour rgb is closest to,
    // never takes its gradient from the cancelling difference c_k - rgb.  Where delta is not clamped the sum equals u_amax (rgb is
    // homogeneous of degree 0 in (w, delta): m cancels).  The sum is compensated (Kahan): K - 1 terms of one size leave one of them.
    // Fragment amax's gradients therefore leave last, when the sum is complete: its g_dist and g_bary wait in registers.
    float u_others = s.m_passes && s.draw >= BLEND_EPS ? g_delta * s.draw / c.gamma : 0.0f, u_comp = 0.0f;
    float held_d = 0.0f, held_b[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < s.n; k++) {
        float p, q, col[D], d, bw[3] = {1.0f, 1.0f, 1.0f}, gb[3] = {0.0f, 0.0f, 0.0f};
        fr.template shade<!UNIT>(k, d, bw);
        sigmoid_pq(d, c.sigma, p, q);
        const float e = expf((zinv_of(fr.z(k), c) - s.m) / c.gamma), w = p * e;
        const int64_t f = fr.face(k);
        const float* fa = attr + (size_t)f * 3 * D;
        frag_colour<D, UNIT>(fa, bw, col);
        float g_w = 0.0f;
#pragma unroll
        for (int ch = 0; ch < D; ch++) g_w += gn[ch] * (col[ch] - rgb[ch]);
        const float u = g_w * w / c.gamma;
        const bool hold = k == s.amax && s.m_passes;
        if (!hold) {
            const float y = u - u_comp, t = u_others + y;
            u_comp = (t - u_others) - y;
            u_others = t;
        }
        const float gd = -((g_alpha * s.q.without(q) + g_w * e) * (p * q)) / c.sigma;
#pragma unroll
        for (int ch = 0; ch < D; ch++) {
            const float g_c = gn[ch] * w;  // dL/dc_kc
#pragma unroll
            for (int j = 0; j < 3; j++) {
                gb[j] += g_c * fa[j * D + ch];
                const float ga = bw[j] * g_c;
                if (g_attr && ga != 0.0f) atomicAdd(&g_attr[(size_t)f * 3 * D + j * D + ch], ga);
            }
        }
        if (UNIT) gb[0] = gb[1] = gb[2] = 0.0f;  // the weights are constants
        if (hold) held_d = gd, held_b[0] = gb[0], held_b[1] = gb[1], held_b[2] = gb[2];
        else sink.emit(k, f, -u / c.zrange, gb, gd);  // zinv = (zfar - z) / zrange
    }
    if (s.m_passes) sink.emit(s.amax, fr.face(s.amax), u_others / c.zrange, held_b, held_d);
}

// FOHO_RASTK_BLEND_ALPHA_ONLY: alpha = 1 - prod_k q_k from the distances alone.  The product; returns the pixel's fragments
template <class FRAGS>
__device__ __forceinline__ int alpha_prod(const FRAGS& fr, float sigma, QProd& pr) {
    pr.pnz = 1.0f, pr.nzero = 0;
    int n = 0;
    for (; fr.has(n); n++) {
        float p, q, d;
        fr.template shade<false>(n, d, nullptr);
        sigmoid_pq(d, sigma, p, q);
        pr.mul(q);
    }
    return n;
}
template <class FRAGS, class SINK>
__device__ __forceinline__ void alpha_grads(const FRAGS& fr, int n, const QProd& pr, float sigma, float g_alpha, const SINK& sink) {
    const float none[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < n; k++) {
        float p, q, d;
        fr.template shade<false>(k, d, nullptr);
        sigmoid_pq(d, sigma, p, q);
        sink.emit(k, fr.face(k), 0.0f, none, -((g_alpha * pr.without(q)) * (p * q)) / sigma);
    }
}

template <int D, bool UNIT>
__global__ __launch_bounds__(TPB) void k_rk_blend_fwd(const int64_t* __restrict__ p2f, const float* __restrict__ zbuf, const float* __restrict__ bary,
                                                      const float* __restrict__ dists, const float* __restrict__ attr, BlendCfg c,
                                                      float* __restrict__ out) {
    const size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (pix >= c.pixels) return;
    const size_t o = pix * (size_t)c.K;
    const PlaneFrags fr = {p2f + o, zbuf + o, UNIT ? nullptr : bary + 3 * o, dists + o, c.K, c.F};
    write_pixel<D>(pixel_sums<D, UNIT>(fr, attr, c), c, out + pix * (D + 1));
}

template <int D, bool UNIT>
__global__ __launch_bounds__(TPB) void k_rk_blend_bwd(const int64_t* __restrict__ p2f, const float* __restrict__ zbuf, const float* __restrict__ bary,
                                                      const float* __restrict__ dists, const float* __restrict__ attr, BlendCfg c,
                                                      const float* __restrict__ g_out, float* __restrict__ g_z, float* __restrict__ g_b,
                                                      float* __restrict__ g_d, float* g_attr) {
    const size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (pix >= c.pixels) return;
    const size_t o = pix * (size_t)c.K;
    const PlaneFrags fr = {p2f + o, zbuf + o, UNIT ? nullptr : bary + 3 * o, dists + o, c.K, c.F};
    if (!fr.has(0)) return;  // no fragment: nothing depends on the planes
    const PlaneSink sink = {g_z ? g_z + o : nullptr, !UNIT && g_b ? g_b + 3 * o : nullptr, g_d ? g_d + o : nullptr};
    pixel_grads<D, UNIT>(fr, pixel_sums<D, UNIT>(fr, attr, c), attr, c, g_out + pix * (D + 1), sink, g_attr);
}

// FOHO_RASTK_BLEND_ALPHA_ONLY: out (H,W) = 1 - prod_k q_k; only the ids and the distances are read, and a negative id alone ends a pixel
__global__ __launch_bounds__(TPB) void k_rk_alpha_fwd(const int64_t* __restrict__ p2f, const float* __restrict__ dists, BlendCfg c, float* __restrict__ out) {
    const size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (pix >= c.pixels) return;
    const size_t o = pix * (size_t)c.K;
    const PlaneFrags fr = {p2f + o, nullptr, nullptr, dists + o, c.K, INT64_MAX};
    QProd pr;
    alpha_prod(fr, c.sigma, pr);
    out[pix] = 1.0f - pr.full();
}

__global__ __launch_bounds__(TPB) void k_rk_alpha_bwd(const int64_t* __restrict__ p2f, const float* __restrict__ dists, BlendCfg c,
                                                      const float* __restrict__ g_out, float* __restrict__ g_d) {
    const size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (pix >= c.pixels) return;
    const size_t o = pix * (size_t)c.K;
    const PlaneFrags fr = {p2f + o, nullptr, nullptr, dists + o, c.K, INT64_MAX};
    QProd pr;
    const int n = alpha_prod(fr, c.sigma, pr);
    const PlaneSink sink = {nullptr, nullptr, g_d + o};
    alpha_grads(fr, n, pr, c.sigma, g_out[pix], sink);
}

// the checks both entry points share; 0 or the refusal's status
// ... the part of them that needs no plane: flags, K, D, the frame, the scalars (foho_rastk_render_* checks these too)
int blend_scalars(const std::string& who, int32_t F, int32_t H, int32_t W, int32_t K, int32_t D, float sigma, float gamma, float znear, float zfar,
                  int32_t flags) {
    if (flags & ~(FOHO_RASTK_BLEND_UNIT_BARY | FOHO_RASTK_BLEND_ALPHA_ONLY)) return fail(-1, who + "unknown flag");
    const bool alpha = flags & FOHO_RASTK_BLEND_ALPHA_ONLY;
    if (!k_ok(K)) return fail(-1, who + "K outside 1 .. 128");
    if (D < 1 || D > FOHO_RASTK_BLEND_MAX_D) return fail(-1, who + "D outside 1 .. 4");
    if (!dims_ok(1, alpha ? 1 : F, H, W)) return fail(-1, who + "F, H or W out of range");
    if (!(sigma > 0.0f)) return fail(-1, who + "sigma must be positive");
    if (!alpha && !(gamma > 0.0f)) return fail(-1, who + "gamma must be positive");
    if (!alpha && !(zfar > znear)) return fail(-1, who + "zfar must exceed znear");
    return 0;
}
void blend_cfg(BlendCfg& c, int32_t F, int32_t H, int32_t W, int32_t K, int32_t D, float sigma, float gamma, float znear, float zfar,
               const float* background, int32_t flags) {
    const bool alpha = flags & FOHO_RASTK_BLEND_ALPHA_ONLY;
    c.sigma = sigma, c.gamma = gamma, c.zfar = zfar, c.zrange = zfar - znear;
    for (int ch = 0; ch < 4; ch++) c.bg[ch] = (!alpha && ch < D) ? background[ch] : 0.0f;
    c.K = K, c.F = F, c.pixels = (size_t)H * W;
}
int blend_args(const char* fn, const int64_t* p2f, const float* zbuf, const float* bary, const float* dists, const float* attr, int32_t F,
               int32_t H, int32_t W, int32_t K, int32_t D, float sigma, float gamma, float znear, float zfar, const float* background,
               int32_t flags, BlendCfg& c) {
    const std::string who = std::string(fn) + ": ";
    const int bad = blend_scalars(who, F, H, W, K, D, sigma, gamma, znear, zfar, flags);
    if (bad) return bad;
    const bool alpha = flags & FOHO_RASTK_BLEND_ALPHA_ONLY, unit = flags & FOHO_RASTK_BLEND_UNIT_BARY;
    if (!p2f || !dists || (!alpha && (!zbuf || !attr || !background || (!unit && !bary)))) return fail(-1, who + "null argument");
    blend_cfg(c, F, H, W, K, D, sigma, gamma, znear, zfar, background, flags);
    return 0;
}

// one instance per (D, unit weights)
#define RK_BLEND_DISPATCH(KERNEL, D, unit, ...)                                                                   \
    do {                                                                                                          \
        const dim3 grid(blocks_for(c.pixels, TPB)), block(TPB);                                                   \
        const hipStream_t st = (hipStream_t)stream;                                                               \
        switch ((D) * 2 + ((unit) ? 1 : 0)) {                                                                     \
            case 2: hipLaunchKernelGGL((KERNEL<1, false>), grid, block, 0, st, __VA_ARGS__); break;              \
            case 3: hipLaunchKernelGGL((KERNEL<1, true>), grid, block, 0, st, __VA_ARGS__); break;               \
            case 4: hipLaunchKernelGGL((KERNEL<2, false>), grid, block, 0, st, __VA_ARGS__); break;              \
            case 5: hipLaunchKernelGGL((KERNEL<2, true>), grid, block, 0, st, __VA_ARGS__); break;               \
            case 6: hipLaunchKernelGGL((KERNEL<3, false>), grid, block, 0, st, __VA_ARGS__); break;              \
            case 7: hipLaunchKernelGGL((KERNEL<3, true>), grid, block, 0, st, __VA_ARGS__); break;               \
            case 8: hipLaunchKernelGGL((KERNEL<4, false>), grid, block, 0, st, __VA_ARGS__); break;              \
            default: hipLaunchKernelGGL((KERNEL<4, true>), grid, block, 0, st, __VA_ARGS__); break;              \
        }                                                                                                         \
    } while (0)

}  // namespace

extern "C" {

FOHO_RASTK_API int foho_rastk_blend_fwd(const int64_t* pix_to_face, const float* zbuf, const float* bary, const float* dists,
                                        const float* face_attr, int32_t F, int32_t H, int32_t W, int32_t K, int32_t D, float sigma,
                                        float gamma, float znear, float zfar, const float* background, int32_t flags, float* out,
                                        void* stream) {
    BlendCfg c;
    const int bad = blend_args("foho_rastk_blend_fwd", pix_to_face, zbuf, bary, dists, face_attr, F, H, W, K, D, sigma, gamma, znear, zfar,
                               background, flags, c);
    if (bad) return bad;
    if (!out) return fail(-1, "foho_rastk_blend_fwd: null argument");
    if (flags & FOHO_RASTK_BLEND_ALPHA_ONLY)
        hipLaunchKernelGGL(k_rk_alpha_fwd, dim3(blocks_for(c.pixels, TPB)), dim3(TPB), 0, (hipStream_t)stream, pix_to_face, dists, c, out);
    else
        RK_BLEND_DISPATCH(k_rk_blend_fwd, D, flags & FOHO_RASTK_BLEND_UNIT_BARY, pix_to_face, zbuf, bary, dists, face_attr, c, out);
    return launched("foho_rastk_blend_fwd");
}

FOHO_RASTK_API int foho_rastk_blend_bwd(const int64_t* pix_to_face, const float* zbuf, const float* bary, const float* dists,
                                        const float* face_attr, int32_t F, int32_t H, int32_t W, int32_t K, int32_t D, float sigma,
                                        float gamma, float znear, float zfar, const float* background, int32_t flags,
                                        const float* grad_out, float* grad_zbuf, float* grad_bary, float* grad_dists,
                                        float* grad_face_attr, void* stream) {
    BlendCfg c;
    const int bad = blend_args("foho_rastk_blend_bwd", pix_to_face, zbuf, bary, dists, face_attr, F, H, W, K, D, sigma, gamma, znear, zfar,
                               background, flags, c);
    if (bad) return bad;
    if (!grad_out) return fail(-1, "foho_rastk_blend_bwd: null argument");
    if (flags & FOHO_RASTK_BLEND_ALPHA_ONLY) {
        if (!grad_dists) return 0;  // alpha depends on the distances alone
        hipLaunchKernelGGL(k_rk_alpha_bwd, dim3(blocks_for(c.pixels, TPB)), dim3(TPB), 0, (hipStream_t)stream, pix_to_face, dists, c, grad_out,
                           grad_dists);
    } else {
        if (!grad_zbuf && !grad_bary && !grad_dists && !grad_face_attr) return 0;
        RK_BLEND_DISPATCH(k_rk_blend_bwd, D, flags & FOHO_RASTK_BLEND_UNIT_BARY, pix_to_face, zbuf, bary, dists, face_attr, c, grad_out,
                          grad_zbuf, grad_bary, grad_dists, grad_face_attr);
    }
    return launched("foho_rastk_blend_bwd");
}

}  // extern "C"
#undef RK_BLEND_DISPATCH
