// rastk_blend.inc -- foho_rastk_blend_fwd / _bwd (foho_rastk.h): interpolate_face_attributes + softmax_rgb_blend over the K planes
// foho_rastk_fwd writes, one launch each way.  Included by foho_rastk.hip behind its entry points (fail / launched / blocks_for / TPB
// are foho_side.h's).  DESIGN.md section 3C.
//
// One thread per pixel, no LDS, no workspace.  The planes are front-packed: a pixel's fragments are its n leading entries with an id
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

// sweeps A and B of one pixel (id, z, d: the pixel's K entries; b: its 3 K barycentrics)
template <int D, bool UNIT>
__device__ __forceinline__ PixSums<D> pixel_sums(const int64_t* __restrict__ id, const float* __restrict__ z, const float* __restrict__ b,
                                                 const float* __restrict__ d, const float* __restrict__ attr, const BlendCfg& c) {
    PixSums<D> s;
    s.n = 0, s.amax = 0;
    float zmax = 0.0f;
    for (int k = 0; k < c.K; k++) {
        const int64_t f = id[k];
        if (f < 0 || f >= c.F) break;
        const float zi = zinv_of(z[k], c);
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
        float p, q, col[D];
        sigmoid_pq(d[k], c.sigma, p, q);
        s.q.mul(q);
        const float w = p * expf((zinv_of(z[k], c) - s.m) / c.gamma);
        frag_colour<D, UNIT>(attr + (size_t)id[k] * 3 * D, UNIT ? nullptr : b + 3 * k, col);
        s.S += w;
#pragma unroll
        for (int ch = 0; ch < D; ch++) s.num[ch] += w * col[ch];
    }
    return s;
}

template <int D, bool UNIT>
__global__ __launch_bounds__(TPB) void k_rk_blend_fwd(const int64_t* __restrict__ p2f, const float* __restrict__ zbuf, const float* __restrict__ bary,
                                                      const float* __restrict__ dists, const float* __restrict__ attr, BlendCfg c,
                                                      float* __restrict__ out) {
    const size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (pix >= c.pixels) return;
    const size_t o = pix * (size_t)c.K;
    const PixSums<D> s = pixel_sums<D, UNIT>(p2f + o, zbuf + o, UNIT ? nullptr : bary + 3 * o, dists + o, attr, c);
    float* po = out + pix * (D + 1);
    const float den = s.S + s.delta;
#pragma unroll
    for (int ch = 0; ch < D; ch++) po[ch] = (s.num[ch] + s.delta * c.bg[ch]) / den;  // no fragment: (0 + 1 bg) / 1
    po[D] = 1.0f - s.q.full();
}

template <int D, bool UNIT>
__global__ __launch_bounds__(TPB) void k_rk_blend_bwd(const int64_t* __restrict__ p2f, const float* __restrict__ zbuf, const float* __restrict__ bary,
                                                      const float* __restrict__ dists, const float* __restrict__ attr, BlendCfg c,
                                                      const float* __restrict__ g_out, float* __restrict__ g_z, float* __restrict__ g_b,
                                                      float* __restrict__ g_d, float* g_attr) {
    const size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (pix >= c.pixels) return;
    const size_t o = pix * (size_t)c.K;
    const int64_t* id = p2f + o;
    if (id[0] < 0 || id[0] >= c.F) return;  // no fragment: nothing depends on the planes
    const float *z = zbuf + o, *d = dists + o, *b = UNIT ? nullptr : bary + 3 * o;
    const PixSums<D> s = pixel_sums<D, UNIT>(id, z, b, d, attr, c);
    const float den = s.S + s.delta;
    // rgb_c = (num_c + delta bg_c) / den: gn_c = dL/dnum_c; dL/dw_k = sum_c gn_c (c_kc - rgb_c); dL/ddelta = sum_c gn_c (bg_c - rgb_c)
    float gn[D], rgb[D], g_delta = 0.0f;
#pragma unroll
    for (int ch = 0; ch < D; ch++) {
        rgb[ch] = (s.num[ch] + s.delta * c.bg[ch]) / den;
        gn[ch] = g_out[pix * (D + 1) + ch] / den;
        g_delta += gn[ch] * (c.bg[ch] - rgb[ch]);
    }
    const float g_alpha = g_out[pix * (D + 1) + D];  // out alpha = 1 - prod q: d alpha / d p_k = prod_{j != k} q_j
    // m enters every exponent and, where delta is not clamped, delta.  With u_k = dL/d(zinv_k - m) = dL/dw_k w_k / gamma the max's
    // gradient is -(sum_k u_k + v), v = dL/ddelta delta / gamma where delta is not clamped and 0 where it is, and torch sends it to
    // fragment amax, whose own u cancels: it receives -(sum_{k != amax} u_k + v), summed WITHOUT that term.  So a pixel's only
    // fragment gets exactly -v (0 where delta is clamped, as in torch), and the nearest fragment, whose colour rgb is closest to,
    // never takes its gradient from the cancelling difference c_k - rgb.  Where delta is not clamped the sum equals u_amax (rgb is
    // homogeneous of degree 0 in (w, delta): m cancels).  The sum is compensated (Kahan): K - 1 terms of one size leave one of them.
    float u_others = s.m_passes && s.draw >= BLEND_EPS ? g_delta * s.draw / c.gamma : 0.0f, u_comp = 0.0f;
    for (int k = 0; k < s.n; k++) {
        float p, q, col[D];
        sigmoid_pq(d[k], c.sigma, p, q);
        const float e = expf((zinv_of(z[k], c) - s.m) / c.gamma), w = p * e;
        const float* fa = attr + (size_t)id[k] * 3 * D;
        frag_colour<D, UNIT>(fa, b ? b + 3 * k : nullptr, col);
        float g_w = 0.0f;
#pragma unroll
        for (int ch = 0; ch < D; ch++) g_w += gn[ch] * (col[ch] - rgb[ch]);
        const float u = g_w * w / c.gamma;
        if (k != s.amax || !s.m_passes) {
            if (g_z) g_z[o + k] = -u / c.zrange;  // zinv = (zfar - z) / zrange
            const float y = u - u_comp, t = u_others + y;
            u_comp = (t - u_others) - y;
            u_others = t;
        }
        if (g_d) g_d[o + k] = -((g_alpha * s.q.without(q) + g_w * e) * (p * q)) / c.sigma;
        float bw[3] = {1.0f, 1.0f, 1.0f}, gb[3] = {0.0f, 0.0f, 0.0f};
        if (!UNIT) bw[0] = b[3 * k], bw[1] = b[3 * k + 1], bw[2] = b[3 * k + 2];
#pragma unroll
        for (int ch = 0; ch < D; ch++) {
            const float g_c = gn[ch] * w;  // dL/dc_kc
#pragma unroll
            for (int j = 0; j < 3; j++) {
                gb[j] += g_c * fa[j * D + ch];
                const float ga = bw[j] * g_c;
                if (g_attr && ga != 0.0f) atomicAdd(&g_attr[(size_t)id[k] * 3 * D + j * D + ch], ga);
            }
        }
        if (!UNIT && g_b) g_b[3 * (o + k)] = gb[0], g_b[3 * (o + k) + 1] = gb[1], g_b[3 * (o + k) + 2] = gb[2];
    }
    if (s.m_passes && g_z) g_z[o + s.amax] = u_others / c.zrange;
}

// FOHO_RASTK_BLEND_ALPHA_ONLY: out (H,W) = 1 - prod_k q_k; only the ids and the distances are read
__global__ __launch_bounds__(TPB) void k_rk_alpha_fwd(const int64_t* __restrict__ p2f, const float* __restrict__ dists, BlendCfg c, float* __restrict__ out) {
    const size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (pix >= c.pixels) return;
    const size_t o = pix * (size_t)c.K;
    QProd pr = {1.0f, 0};
    for (int k = 0; k < c.K && p2f[o + k] >= 0; k++) {
        float p, q;
        sigmoid_pq(dists[o + k], c.sigma, p, q);
        pr.mul(q);
    }
    out[pix] = 1.0f - pr.full();
}

__global__ __launch_bounds__(TPB) void k_rk_alpha_bwd(const int64_t* __restrict__ p2f, const float* __restrict__ dists, BlendCfg c,
                                                      const float* __restrict__ g_out, float* __restrict__ g_d) {
    const size_t pix = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (pix >= c.pixels) return;
    const size_t o = pix * (size_t)c.K;
    QProd pr = {1.0f, 0};
    int n = 0;
    for (; n < c.K && p2f[o + n] >= 0; n++) {
        float p, q;
        sigmoid_pq(dists[o + n], c.sigma, p, q);
        pr.mul(q);
    }
    const float g_alpha = g_out[pix];
    for (int k = 0; k < n; k++) {
        float p, q;
        sigmoid_pq(dists[o + k], c.sigma, p, q);
        g_d[o + k] = -((g_alpha * pr.without(q)) * (p * q)) / c.sigma;
    }
}

// the checks both entry points share; 0 or the refusal's status
int blend_args(const char* fn, const int64_t* p2f, const float* zbuf, const float* bary, const float* dists, const float* attr, int32_t F,
               int32_t H, int32_t W, int32_t K, int32_t D, float sigma, float gamma, float znear, float zfar, const float* background,
               int32_t flags, BlendCfg& c) {
    const std::string who = std::string(fn) + ": ";
    if (flags & ~(FOHO_RASTK_BLEND_UNIT_BARY | FOHO_RASTK_BLEND_ALPHA_ONLY)) return fail(-1, who + "unknown flag");
    const bool alpha = flags & FOHO_RASTK_BLEND_ALPHA_ONLY, unit = flags & FOHO_RASTK_BLEND_UNIT_BARY;
    if (!k_ok(K)) return fail(-1, who + "K outside 1 .. 128");
    if (D < 1 || D > FOHO_RASTK_BLEND_MAX_D) return fail(-1, who + "D outside 1 .. 4");
    if (!dims_ok(1, alpha ? 1 : F, H, W)) return fail(-1, who + "F, H or W out of range");
    if (!(sigma > 0.0f)) return fail(-1, who + "sigma must be positive");
    if (!alpha && !(gamma > 0.0f)) return fail(-1, who + "gamma must be positive");
    if (!alpha && !(zfar > znear)) return fail(-1, who + "zfar must exceed znear");
    if (!p2f || !dists || (!alpha && (!zbuf || !attr || !background || (!unit && !bary)))) return fail(-1, who + "null argument");
    c.sigma = sigma, c.gamma = gamma, c.zfar = zfar, c.zrange = zfar - znear;
    for (int ch = 0; ch < 4; ch++) c.bg[ch] = (!alpha && ch < D) ? background[ch] : 0.0f;
    c.K = K, c.F = F, c.pixels = (size_t)H * W;
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
