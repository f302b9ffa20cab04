// foho_side.h -- what the side libraries (libfoho_vol.so, libfoho_sflexi.so, libfoho_rastk.so, libfoho_wflexi.so, libfoho_mreg.so) share.  Internal: everything is in an
// anonymous namespace, so a library that includes it exports nothing new.
//
// Host: the error string behind foho_<name>_last_error, fail / launched, blocks_for, and FOHO_SIDE_ENTRY_POINTS for the version and
// last-error entry points.  Device: gid, usable_count, the workgroup scan, and the mask-word helpers (64 points per word, a wave owns a word).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace {

constexpr int TPB = 256;  // workgroup of the one-thread-per-item kernels: 4 waves, each the owner of one 64-bit mask word

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// after the last launch of an entry point
int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-2, std::string(what) + ": launch failed: " + hipGetErrorString(e));
    return 0;
}

unsigned blocks_for(size_t n, int per = TPB) { return (unsigned)(n ? (n + per - 1) / per : 1); }

// foho_<name>_version and foho_<name>_last_error (declared in foho_<name>.h)
#define FOHO_SIDE_ENTRY_POINTS(name, API, VERSION)                                     \
    extern "C" API int foho_##name##_version(void) { return VERSION; }                 \
    extern "C" API const char* foho_##name##_last_error(void) { return g_err.c_str(); }

__device__ __forceinline__ int64_t gid() { return (int64_t)blockIdx.x * TPB + threadIdx.x; }

// a count an earlier kernel left on the device, as far as the buffers carved for `cap` items can be trusted with it: n when
// 0 <= n <= cap, else 0 (an overflow, or a workspace of another field)
__device__ __forceinline__ int usable_count(int n, int cap) { return (n < 0 || n > cap) ? 0 : n; }

// exclusive scan over the N threads of a workgroup in LDS (Hillis-Steele; s: N items): this thread's exclusive prefix.  The inclusive
// sums stay in s behind the last barrier (the workgroup's total is s[N - 1]).
template <int N, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const T t = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    return s[threadIdx.x] - v;
}
// ... and the workgroup's total to *s_tot, readable by every thread (one more barrier), so that s may be written again at once
template <int N, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* s, T* s_tot) {
    const T ex = block_exclusive_scan<N, T>(v, s);
    if (threadIdx.x == N - 1) *s_tot = ex + v;
    __syncthreads();
    return ex;
}

// the wave's predicate bits become word (first point of the wave) / 64 of the mask over n points, by one store from lane 0, and are
// returned; lanes past n must pass pred = false, so that the last word's upper bits are clear
__device__ __forceinline__ uint64_t store_word(uint64_t* m, int64_t p, int64_t n, bool pred) {
    const uint64_t w = __ballot(pred);
    const int64_t p0 = p - (threadIdx.x & 63);
    if ((threadIdx.x & 63) == 0 && p0 < n) m[p0 >> 6] = w;
    return w;
}

// word w of a mask over n_points, its bits at and past n_points cleared; 0 (and no load) for a word past the mask
__device__ __forceinline__ uint64_t clipped_word(const uint64_t* m, int64_t w, int64_t n_points) {
    const int64_t left = n_points - w * 64;
    if (left <= 0) return 0;
    return left >= 64 ? m[w] : (m[w] & ((1ull << left) - 1));
}

// f(b) for every set bit b of m, ascending
template <typename F>
__device__ __forceinline__ void for_each_bit(uint64_t m, F f) {
    while (m) {
        f(__ffsll((unsigned long long)m) - 1);
        m &= m - 1;
    }
}

}  // namespace
