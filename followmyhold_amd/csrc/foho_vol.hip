// foho_vol.hip -- libfoho_vol.so: index and field kernels of the hierarchical final decode (foho_vol.h, volume.py).
//
// All of it is memory-bound bit and float shuffling over grids of up to 385^3 points (228 MB of float32 field, 7 MB of point mask).
// One thread per point or cell, 256-thread workgroups, so that the 64 lanes of a wave own exactly one 64-bit mask word: a mask is
// written by __ballot and one store from lane 0, never by atomics.  Compaction (foho_vol_count / _emit) is two-pass: popcounts per
// workgroup, one exclusive scan, then each thread writes the set bits of its word in ascending order -- sorted, repeatable.
// Compiled with -ffp-contract=off: the midpoint means of foho_vol_fill are plain binary32 sums in a fixed order, which the numpy
// restatement (tests/vol_ref.py) reproduces bit for bit.
// The error plumbing, gid, the workgroup scan and the mask-word helpers are foho_side.h's.
#include "foho_side.h"
#include "foho_vol.h"

namespace {

constexpr int SCAN_TPB = 1024;

__device__ __forceinline__ bool bit_of(const uint64_t* m, int64_t p) { return (m[p >> 6] >> (p & 63)) & 1ull; }

// any set bit of the cell mask (r^3) in the box [i0, i1] x [j0, j1] x [k0, k1] (already clipped)
__device__ __forceinline__ bool any_in_box(const uint64_t* m, int r, int i0, int i1, int j0, int j1, int k0, int k1) {
    for (int i = i0; i <= i1; i++)
        for (int j = j0; j <= j1; j++)
            for (int k = k0; k <= k1; k++)
                if (bit_of(m, ((int64_t)i * r + j) * r + k)) return true;
    return false;
}

__global__ __launch_bounds__(TPB) void k_vol_mixed(const float* __restrict__ f, int r, uint64_t* __restrict__ mixed) {
    const int64_t p = gid(), n = (int64_t)r * r * r;
    bool m = false;
    if (p < n) {
        const int k = (int)(p % r), j = (int)((p / r) % r), i = (int)(p / ((int64_t)r * r));
        const int64_t G = r + 1;
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) cnt += f[((i + (c >> 2)) * G + j + ((c >> 1) & 1)) * G + k + (c & 1)] > 0.0f;
        m = cnt != 0 && cnt != 8;
    }
    store_word(mixed, p, n, m);
}

__global__ __launch_bounds__(TPB) void k_vol_dilate(const uint64_t* __restrict__ src, int r, int band, uint64_t* __restrict__ dst) {
    const int64_t p = gid(), n = (int64_t)r * r * r;
    bool a = false;
    if (p < n) {
        const int k = (int)(p % r), j = (int)((p / r) % r), i = (int)(p / ((int64_t)r * r));
        a = any_in_box(src, r, max(i - band, 0), min(i + band, r - 1), max(j - band, 0), min(j + band, r - 1), max(k - band, 0),
                       min(k + band, r - 1));
    }
    store_word(dst, p, n, a);
}

// the cells (r^3) a point of the (2r+1)^3 level lies in, along one axis: I even -> I/2 - 1 and I/2, odd -> (I-1)/2; clipped
__device__ __forceinline__ int cell_lo(int I) { return max((I - 1) >> 1, 0); }
__device__ __forceinline__ int cell_hi(int I, int r) { return min(I >> 1, r - 1); }

__global__ __launch_bounds__(TPB) void k_vol_select(const uint64_t* __restrict__ active, const uint64_t* __restrict__ cdec, int r,
                                                    uint64_t* __restrict__ sel, uint64_t* __restrict__ fdec) {
    const int64_t F = 2 * r + 1, p = gid(), n = F * F * F;
    bool s = false, d = false;
    if (p < n) {
        const int K = (int)(p % F), J = (int)((p / F) % F), I = (int)(p / (F * F));
        const int64_t G = r + 1;
        const bool carried = !((I | J | K) & 1) && bit_of(cdec, ((int64_t)(I >> 1) * G + (J >> 1)) * G + (K >> 1));
        s = !carried && any_in_box(active, r, cell_lo(I), cell_hi(I, r), cell_lo(J), cell_hi(J, r), cell_lo(K), cell_hi(K, r));
        d = s || carried;
    }
    store_word(sel, p, n, s);
    store_word(fdec, p, n, d);
}

// cubes (R^3) whose corners are mixed and not all decoded
__global__ __launch_bounds__(TPB) void k_vol_bad(const float* __restrict__ f, const uint64_t* __restrict__ dec, int R,
                                                 uint64_t* __restrict__ bad) {
    const int64_t p = gid(), n = (int64_t)R * R * R;
    bool b = false;
    if (p < n) {
        const int k = (int)(p % R), j = (int)((p / R) % R), i = (int)(p / ((int64_t)R * R));
        const int64_t G = R + 1;
        int cnt = 0;
        bool all_dec = true;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int64_t q = ((i + (c >> 2)) * G + j + ((c >> 1) & 1)) * G + k + (c & 1);
            cnt += f[q] > 0.0f;
            all_dec = all_dec && bit_of(dec, q);
        }
        b = cnt != 0 && cnt != 8 && !all_dec;
    }
    store_word(bad, p, n, b);
}

// undecoded corners of the cubes in `near` (or every undecoded point); decoded |= sel in place: each word is read and written
// by the one wave that owns it
__global__ __launch_bounds__(TPB) void k_vol_close_select(const uint64_t* __restrict__ near, uint64_t* __restrict__ dec, int R, int all,
                                                          uint64_t* __restrict__ sel) {
    const int64_t G = R + 1, p = gid(), n = G * G * G;
    bool s = false;
    uint64_t old = 0;
    if (p < n) {
        old = dec[p >> 6];
        if (!((old >> (p & 63)) & 1ull)) {
            const int K = (int)(p % G), J = (int)((p / G) % G), I = (int)(p / (G * G));
            s = all || any_in_box(near, R, max(I - 1, 0), min(I, R - 1), max(J - 1, 0), min(J, R - 1), max(K - 1, 0), min(K, R - 1));
        }
    }
    const uint64_t w = store_word(sel, p, n, s);
    if ((threadIdx.x & 63) == 0 && p < n) dec[p >> 6] = old | w;
}

// one mask word per thread
__global__ __launch_bounds__(TPB) void k_vol_count(const uint64_t* __restrict__ sel, int64_t n_points, int32_t* __restrict__ bsum) {
    __shared__ int s[TPB];
    __shared__ int tot;
    const int64_t w = gid();
    block_exclusive_scan<TPB, int>(__popcll(clipped_word(sel, w, n_points)), s, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one workgroup: in-place exclusive scan of nb block counts, the total to *total
__global__ __launch_bounds__(SCAN_TPB) void k_vol_scan(int32_t* __restrict__ b, int nb, int32_t* __restrict__ total) {
    __shared__ int s[SCAN_TPB];
    __shared__ int tot;
    const int per = (nb + SCAN_TPB - 1) / SCAN_TPB;
    const int lo = min((int)threadIdx.x * per, nb), hi = min(lo + per, nb);
    int v = 0;
    for (int q = lo; q < hi; q++) v += b[q];
    int run = block_exclusive_scan<SCAN_TPB>(v, s, &tot);
    for (int q = lo; q < hi; q++) {
        const int x = b[q];
        b[q] = run;
        run += x;
    }
    if (threadIdx.x == 0) *total = tot;
}

__global__ __launch_bounds__(TPB) void k_vol_emit(const uint64_t* __restrict__ sel, int r, int stride, int R, const float* __restrict__ tab,
                                                  const int32_t* __restrict__ boff, int32_t* __restrict__ idx, float* __restrict__ xyz) {
    __shared__ int s[TPB];
    __shared__ int tot;
    const int64_t G = r + 1, n_points = G * G * G, w = gid();
    const uint64_t m = clipped_word(sel, w, n_points);
    int o = boff[blockIdx.x] + block_exclusive_scan<TPB, int>(__popcll(m), s, &tot);
    const int64_t T = R + 1;
    for_each_bit(m, [&](int b) {
        const int64_t p = w * 64 + b;
        const int k = (int)(p % G), j = (int)((p / G) % G), i = (int)(p / (G * G));
        idx[o] = (int32_t)p;
        xyz[3 * (int64_t)o + 0] = tab[(int64_t)i * stride];
        xyz[3 * (int64_t)o + 1] = tab[T + (int64_t)j * stride];
        xyz[3 * (int64_t)o + 2] = tab[2 * T + (int64_t)k * stride];
        o++;
    });
}

// value at even indices, else the mean of the 2 / 4 / 8 enclosing coarse corners, summed x-corner outermost, z innermost
__global__ __launch_bounds__(TPB) void k_vol_fill(const float* __restrict__ c, int r, float* __restrict__ f) {
    const int64_t F = 2 * r + 1, G = r + 1, p = gid();
    if (p >= F * F * F) return;
    const int K = (int)(p % F), J = (int)((p / F) % F), I = (int)(p / (F * F));
    const int i = I >> 1, j = J >> 1, k = K >> 1, oi = I & 1, oj = J & 1, ok = K & 1;
    float s = 0.0f;
    bool first = true;
    for (int a = 0; a <= oi; a++)
        for (int b = 0; b <= oj; b++)
            for (int d = 0; d <= ok; d++) {
                const float v = c[((int64_t)(i + a) * G + j + b) * G + k + d];
                s = first ? v : s + v;
                first = false;
            }
    const int odd = oi + oj + ok;
    f[p] = odd == 0 ? s : s * (odd == 1 ? 0.5f : (odd == 2 ? 0.25f : 0.125f));
}

__global__ __launch_bounds__(TPB) void k_vol_scatter(const int32_t* __restrict__ idx, const float* __restrict__ v, int64_t n, float* __restrict__ f) {
    const int64_t q = gid();
    if (q < n) f[idx[q]] = v[q];
}

bool res_ok(int32_t r) { return r >= 1 && r <= FOHO_VOL_MAX_RES; }

}  // namespace

FOHO_SIDE_ENTRY_POINTS(vol, FOHO_VOL_API, FOHO_VOL_VERSION)

extern "C" {

FOHO_VOL_API int foho_vol_mark(const float* field, int32_t r, int32_t band, uint64_t* mixed, uint64_t* active, void* stream) {
    if (!field || !mixed || !active) return fail(-1, "foho_vol_mark: null argument");
    if (!res_ok(r) || band < 0 || band > r) return fail(-1, "foho_vol_mark: bad resolution or band");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)r * r * r;
    hipLaunchKernelGGL(k_vol_mixed, dim3(blocks_for(n)), dim3(TPB), 0, st, field, r, mixed);
    hipLaunchKernelGGL(k_vol_dilate, dim3(blocks_for(n)), dim3(TPB), 0, st, mixed, r, band, active);
    return launched("foho_vol_mark");
}

FOHO_VOL_API int foho_vol_select(const uint64_t* active, const uint64_t* coarse_decoded, int32_t r, uint64_t* sel, uint64_t* fine_decoded,
                                 void* stream) {
    if (!active || !coarse_decoded || !sel || !fine_decoded) return fail(-1, "foho_vol_select: null argument");
    if (!res_ok(2 * r)) return fail(-1, "foho_vol_select: bad resolution");
    const int64_t F = 2 * (int64_t)r + 1;
    hipLaunchKernelGGL(k_vol_select, dim3(blocks_for(F * F * F)), dim3(TPB), 0, (hipStream_t)stream, active, coarse_decoded, r, sel, fine_decoded);
    return launched("foho_vol_select");
}

FOHO_VOL_API int foho_vol_close(const float* field, uint64_t* decoded, int32_t R, int32_t mode, uint64_t* bad, uint64_t* near, uint64_t* sel,
                                void* stream) {
    if (!field || !decoded || !sel || (mode == 0 && (!bad || !near))) return fail(-1, "foho_vol_close: null argument");
    if (!res_ok(R) || (mode != 0 && mode != FOHO_VOL_CLOSE_ALL)) return fail(-1, "foho_vol_close: bad resolution or mode");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t nc = (int64_t)R * R * R, G = R + 1;
    if (mode == 0) {
        hipLaunchKernelGGL(k_vol_bad, dim3(blocks_for(nc)), dim3(TPB), 0, st, field, decoded, R, bad);
        hipLaunchKernelGGL(k_vol_dilate, dim3(blocks_for(nc)), dim3(TPB), 0, st, bad, R, 1, near);
    }
    hipLaunchKernelGGL(k_vol_close_select, dim3(blocks_for(G * G * G)), dim3(TPB), 0, st, near, decoded, R, mode, sel);
    return launched("foho_vol_close");
}

FOHO_VOL_API int64_t foho_vol_count_blocks(int64_t n_points) {
    if (n_points < 0) return 0;
    return ((n_points + 63) / 64 + TPB - 1) / TPB;
}

FOHO_VOL_API int foho_vol_count(const uint64_t* sel, int64_t n_points, int32_t* block_offsets, int32_t* total, void* stream) {
    if (!sel || !block_offsets || !total) return fail(-1, "foho_vol_count: null argument");
    if (n_points < 1 || n_points > INT32_MAX) return fail(-1, "foho_vol_count: bad point count");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t nb = foho_vol_count_blocks(n_points);
    hipLaunchKernelGGL(k_vol_count, dim3((unsigned)nb), dim3(TPB), 0, st, sel, n_points, block_offsets);
    hipLaunchKernelGGL(k_vol_scan, dim3(1), dim3(SCAN_TPB), 0, st, block_offsets, (int)nb, total);
    return launched("foho_vol_count");
}

FOHO_VOL_API int foho_vol_emit(const uint64_t* sel, int32_t r, int32_t R, const float* tables, const int32_t* block_offsets, int32_t* idx,
                               float* xyz, void* stream) {
    if (!sel || !tables || !block_offsets || !idx || !xyz) return fail(-1, "foho_vol_emit: null argument");
    if (!res_ok(r) || !res_ok(R) || R % r != 0) return fail(-1, "foho_vol_emit: bad resolution (R must be a multiple of r)");
    const int64_t G = r + 1;
    hipLaunchKernelGGL(k_vol_emit, dim3((unsigned)foho_vol_count_blocks(G * G * G)), dim3(TPB), 0, (hipStream_t)stream, sel, r, R / r, R, tables,
                       block_offsets, idx, xyz);
    return launched("foho_vol_emit");
}

FOHO_VOL_API int foho_vol_fill(const float* coarse, int32_t r, float* fine, void* stream) {
    if (!coarse || !fine) return fail(-1, "foho_vol_fill: null argument");
    if (!res_ok(2 * r)) return fail(-1, "foho_vol_fill: bad resolution");
    const int64_t F = 2 * (int64_t)r + 1;
    hipLaunchKernelGGL(k_vol_fill, dim3(blocks_for(F * F * F)), dim3(TPB), 0, (hipStream_t)stream, coarse, r, fine);
    return launched("foho_vol_fill");
}

FOHO_VOL_API int foho_vol_scatter(const int32_t* idx, const float* vals, int64_t n, float* field, void* stream) {
    if (n < 0 || n > INT32_MAX) return fail(-1, "foho_vol_scatter: bad count");
    if (n == 0) return 0;
    if (!idx || !vals || !field) return fail(-1, "foho_vol_scatter: null argument");
    hipLaunchKernelGGL(k_vol_scatter, dim3(blocks_for(n)), dim3(TPB), 0, (hipStream_t)stream, idx, vals, n, field);
    return launched("foho_vol_scatter");
}

}  // extern "C"
