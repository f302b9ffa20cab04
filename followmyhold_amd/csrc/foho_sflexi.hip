// foho_sflexi.hip -- libfoho_sflexi.so: FlexiCubes from per-axis coordinate tables, on the surface cubes only (foho_sflexi.h,
// sparse_flexi.py).
//
// k_flexi.inc's extractor walks every cube and every grid edge of the (res+1)^3 grid and keeps 9 B per cube + 8 B per edge; it reads
// grid positions only at the 8 corners of the cubes whose corners differ in sign.  Here:
//   k_sf_mark       one thread per cube: sign code of its 8 corners (`s < 0`, as k_flexi_classify); a wave owns one 64-bit mask word
//                   (__ballot, one store); the workgroup's popcount
//   scan            (chunk sums, their scan by one workgroup, apply) exclusive prefix of the popcounts: rank(cube) =
//                   prefix[cube / 256] + popcounts of the words in front of the cube's inside its 256-block + popcount of the lower
//                   bits of its word -- no res^3 int32 table
//   k_sf_compact    ascending list of the surface cubes' ids (one thread per mask word)
//   k_sf_classify   per surface cube: case code, and one flag per axis for the grid edge that starts at the cube's minimum
//                   corner (k_flexi_classify's rule: the two transverse coordinates in 1 .. res-1).  Every quad-owning edge is the
//                   minimum-corner edge of a surface cube, and cube ids ascend in the (i,j,k) order edge ids do
//   scan            ONE exclusive scan over 4n items: n patch counts, then the flags of axis 0, 1, 2 -> vertex offsets by
//                   (cube, patch), quad offsets by (axis, i, j, k): the dense orders.  off[n] is the vertex total
//   k_sf_emit       vertices per surface cube (positions from the tables), quads per (axis, surface cube), the four ring cubes
//                   through rank()
//   k_sf_bwd        dL/ds from dL/dvertices (foho_sflexi_bwd), on what the kernels above left: 8 threads per surface cube, the owner
//                   of a grid point gathers its at most 24 terms in a fixed order and stores once -- no float atomics.  The
//                   ownership rule and the order of the walk are flexi_core.h's, shared with k_wf_bwd_gather; the terms are written here
// Compiled with foho_step.hip's flags (-ffp-contract=off, correctly rounded division and sqrt): the index arithmetic, the sign code,
// the dual vertex and l_dev, the ring table and the quad's orientation and split are flexi_core.h's, the ones k_flexi.inc calls, which
// is what makes the vertices, faces and l_dev bitwise the dense ones.  What is written here is what differs: corner positions from the
// axis tables, offsets and case codes through rank_of on the compact list, the orientation from the case code, the capacity checks.
// The error plumbing, gid, usable_count, the workgroup scan and the mask-word helpers are foho_side.h's; the workspace allocator is
// foho_carve.h's.
#include "flexi_core.h"
#include "foho_carve.h"
#include "foho_side.h"
#include "foho_sflexi.h"

namespace {

constexpr int ITEMS = 2048;  // items per workgroup of the scan (256 threads x 8)

struct MarkWs {
    uint64_t* mask;  // words: bit c % 64 of word c / 64 for cube c
    int32_t* bpre;   // blocks: surface cubes in front of each block of 256 cubes
    int32_t* csum;   // chunks: scan scratch
    int32_t* total;  // surface cubes
    size_t words, blocks, chunks, bytes;
};
MarkWs carve_mark(const void* ws, int res) {
    const size_t C = (size_t)res * res * res;
    MarkWs w;
    w.words = (C + 63) / 64, w.blocks = (C + TPB - 1) / TPB, w.chunks = (w.blocks + ITEMS - 1) / ITEMS;
    char* p = (char*)const_cast<void*>(ws);
    Carve cv;
    w.mask = (uint64_t*)(p + cv.take(w.words * 8));
    w.bpre = (int32_t*)(p + cv.take(w.blocks * 4));
    w.csum = (int32_t*)(p + cv.take(w.chunks * 4));
    w.total = (int32_t*)(p + cv.take(4));
    w.bytes = cv.off;
    return w;
}

struct CubeWs {
    int32_t* cid;  // cap: ascending ids of the surface cubes
    int32_t* off;  // 4 cap: vertex offset per cube, then (vertex total +) quad offset per (axis, cube)
    uint8_t* cse;  // cap: case code
    uint8_t* efl;  // cap: bit a = the axis-a edge at the minimum corner owns a quad
    int32_t* csum;
    int32_t* gtot;  // vertices + quads
    size_t chunks, bytes;
};
CubeWs carve_cube(void* ws, int cap) {
    const size_t n = (size_t)cap;
    CubeWs w;
    w.chunks = (4 * n + ITEMS - 1) / ITEMS;
    char* p = (char*)ws;
    Carve cv;
    w.cid = (int32_t*)(p + cv.take(n * 4));
    w.off = (int32_t*)(p + cv.take(4 * n * 4));
    w.cse = (uint8_t*)(p + cv.take(n));
    w.efl = (uint8_t*)(p + cv.take(n));
    w.csum = (int32_t*)(p + cv.take(w.chunks * 4));
    w.gtot = (int32_t*)(p + cv.take(4));
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(TPB) void k_sf_mark(const float* __restrict__ s, int res, uint64_t* __restrict__ mask, int32_t* __restrict__ bcnt) {
    __shared__ int s_w[TPB / 64];
    const int64_t p = gid(), n = (int64_t)res * res * res;
    bool m = false;
    if (p < n) {
        const unsigned code = flexi_cube_code(s, res, FLEXI_I(p, res), FLEXI_J(p, res), FLEXI_K(p, res));
        m = code != 0u && code != 255u;
    }
    const uint64_t w = store_word(mask, p, n, m);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(w);
    __syncthreads();
    if (threadIdx.x == 0) bcnt[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// the sequence a scan runs over: the int32 array itself (n_host items, in place), or the 4n items of the surface cubes
// (n = *n_dev): patch counts of the n cubes, then their edge flags of axis 0, 1, 2
struct Seq {
    const int32_t* i32;
    int64_t n_host;
    const uint8_t *cse, *efl;
    const int32_t* n_dev;
    int32_t cap;
};
__device__ __forceinline__ int seq_cubes(const Seq& q) {
    if (!q.n_dev) return 0;
    const int n = *q.n_dev;
    return (n < 0 || n > q.cap) ? 0 : n;
}
__device__ __forceinline__ int64_t seq_len(const Seq& q, int n) { return q.n_dev ? 4 * (int64_t)n : q.n_host; }
__device__ __forceinline__ int seq_val(const Seq& q, int64_t t, int n) {
    if (!q.n_dev) return q.i32[t];
    if (t < n) return c_flexi_npatch[q.cse[t]];
    const int64_t u = t - n;
    return (q.efl[u % n] >> (int)(u / n)) & 1;
}

__global__ __launch_bounds__(TPB) void k_sf_sums(Seq q, int32_t* __restrict__ csum) {
    __shared__ int s[TPB];
    const int n = seq_cubes(q);
    const int64_t len = seq_len(q, n), base = (int64_t)blockIdx.x * ITEMS + (int64_t)threadIdx.x * 8;
    if ((int64_t)blockIdx.x * ITEMS >= len) return;
    int v = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) v += (base + e < len) ? seq_val(q, base + e, n) : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int half = TPB / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) csum[blockIdx.x] = s[0];
}

// one workgroup: exclusive scan of the chunk sums in place (TPB at a time, a running carry)
__global__ __launch_bounds__(TPB) void k_sf_scan_chunks(Seq q, int32_t* __restrict__ csum) {
    __shared__ int s[TPB];
    __shared__ int tot;
    const int64_t len = seq_len(q, seq_cubes(q));
    const int nb = (int)((len + ITEMS - 1) / ITEMS);
    int carry = 0;
    for (int base = 0; base < nb; base += TPB) {
        const int i = base + (int)threadIdx.x;
        const int v = i < nb ? csum[i] : 0;
        const int ex = block_exclusive_scan<TPB>(v, s, &tot);
        if (i < nb) csum[i] = carry + ex;
        carry += tot;
        __syncthreads();  // tot is read before the next round's scan writes it
    }
}

// out[t] = items in front of t, from the scanned chunk sums; the grand total goes to *total and, when given, *total2
__global__ __launch_bounds__(TPB) void k_sf_apply(Seq q, const int32_t* __restrict__ csum, int32_t* out, int32_t* __restrict__ total,
                                                  int32_t* __restrict__ total2) {
    __shared__ int s[TPB];
    __shared__ int tot;
    const int n = seq_cubes(q);
    const int64_t len = seq_len(q, n), base = (int64_t)blockIdx.x * ITEMS + (int64_t)threadIdx.x * 8;
    if (len == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        *total = 0;
        if (total2) *total2 = 0;
    }
    if ((int64_t)blockIdx.x * ITEMS >= len) return;
    int v[8], sum = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        v[e] = (base + e < len) ? seq_val(q, base + e, n) : 0;
        sum += v[e];
    }
    int off = csum[blockIdx.x] + block_exclusive_scan<TPB>(sum, s, &tot);
#pragma unroll
    for (int e = 0; e < 8; e++) {
        if (base + e < len) out[base + e] = off;
        off += v[e];
    }
    if ((int64_t)(blockIdx.x + 1) * ITEMS >= len && threadIdx.x == TPB - 1) {  // the last chunk: off = the grand total
        *total = off;
        if (total2) *total2 = off;
    }
}

// surface cubes in front of `cube`
__device__ __forceinline__ int rank_of(const uint64_t* __restrict__ mask, const int32_t* __restrict__ bpre, int64_t cube) {
    const int64_t w = cube >> 6;
    int r = bpre[cube >> 8];
    for (int64_t ww = w & ~(int64_t)3; ww < w; ww++) r += __popcll(mask[ww]);
    return r + __popcll(mask[w] & ((1ull << (cube & 63)) - 1ull));
}

// one mask word per thread: its set bits in ascending order; thread 0 clears the counts
__global__ __launch_bounds__(TPB) void k_sf_compact(const uint64_t* __restrict__ mask, const int32_t* __restrict__ bpre,
                                                    const int32_t* __restrict__ total, int64_t words, int cap, int32_t* __restrict__ cid,
                                                    int32_t* __restrict__ counts) {
    const int64_t w = gid();
    const int n = *total;
    if (w == 0) {
        counts[0] = 0;
        counts[1] = 0;
        counts[2] = (n < 0 || n > cap) ? FOHO_SFLEXI_OVER_CUBES : 0;
    }
    if (w >= words || n < 0 || n > cap) return;
    const uint64_t m = mask[w];
    if (!m) return;
    int o = bpre[w >> 2];
    for (int64_t ww = w & ~(int64_t)3; ww < w; ww++) o += __popcll(mask[ww]);
    for_each_bit(m, [&](int b) {
        if ((unsigned)o < (unsigned)n) cid[o] = (int32_t)(w * 64 + b);  // (a mark buffer of another field cannot write past n)
        o++;
    });
}

__global__ __launch_bounds__(TPB) void k_sf_classify(const float* __restrict__ s, int res, const int32_t* __restrict__ total, int cap,
                                                     const int32_t* __restrict__ cid, uint8_t* __restrict__ cse, uint8_t* __restrict__ efl) {
    const int64_t c = gid();
    const int n = *total;
    if (n < 0 || n > cap || c >= n) return;
    const int64_t cube = cid[c], C = (int64_t)res * res * res;
    unsigned code = 0, f = 0;
    if (cube >= 0 && cube < C) {
        FLEXI_IJK(cube, res)
        code = flexi_cube_code(s, res, i, j, k);
        // the edge from the minimum corner along an axis ends at a grid point (i, j, k < res); it has four cubes around it when
        // its two transverse coordinates are interior; its ends are corners 0 and 1 / 2 / 4
        const bool ii = i >= 1 && i <= res - 1, jj = j >= 1 && j <= res - 1, kk = k >= 1 && k <= res - 1;
        if (jj && kk) f |= (code ^ (code >> 1)) & 1u;
        if (ii && kk) f |= ((code ^ (code >> 2)) & 1u) << 1;
        if (ii && jj) f |= ((code ^ (code >> 4)) & 1u) << 2;
    }
    cse[c] = (uint8_t)code;
    efl[c] = (uint8_t)f;
}

// flexi_verts_role of k_flexi.inc for compact cube c, the corner positions from the axis tables
__device__ __forceinline__ void sf_verts_role(int64_t c, int n, const float* __restrict__ axes, const float* __restrict__ s, int res,
                                              const int32_t* __restrict__ cid, const uint8_t* __restrict__ cse,
                                              const int32_t* __restrict__ off, float* __restrict__ verts, float* __restrict__ ldev, int cap,
                                              int32_t* counts) {
    if (c >= n) return;
    const unsigned code = cse[c];
    const int np = c_flexi_npatch[code];
    if (np == 0) return;
    const int base = off[c];
    if (base < 0 || base + np > cap) {
        atomicOr(&counts[2], FOHO_SFLEXI_OVER_VERTS);
        return;
    }
    const int G = res + 1;
    const int64_t cube = cid[c];
    FLEXI_IJK(cube, res)
    float sc[8], xc[24];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int ci = i + (q & 1), cj = j + ((q >> 1) & 1), ck = k + (q >> 2);
        sc[q] = s[flexi_point(ci, cj, ck, G)];
        xc[3 * q + 0] = axes[ci];
        xc[3 * q + 1] = axes[G + cj];
        xc[3 * q + 2] = axes[2 * G + ck];
    }
    for (int p = 0; p < np; p++) flexi_dual_vertex(code, p, sc, xc, verts + 3 * (size_t)(base + p), ldev ? ldev + (base + p) : nullptr);
}

// flexi_faces_role of k_flexi.inc for item t = axis * n + compact cube: the edge at the cube's minimum corner
__device__ __forceinline__ void sf_faces_role(int64_t t, int n, int res, const uint64_t* __restrict__ mask, const int32_t* __restrict__ bpre,
                                              const int32_t* __restrict__ cid, const uint8_t* __restrict__ cse,
                                              const uint8_t* __restrict__ efl, const int32_t* __restrict__ off, int64_t* __restrict__ faces,
                                              int cap, int32_t* counts) {
    if (t >= 3 * (int64_t)n) return;
    const int axis = (int)(t / n);
    const int64_t c = t % n;
    if (!((efl[c] >> axis) & 1)) return;
    const int qd = off[n + t] - off[n];  // off[n]: the vertex total in front of the first flag
    if (qd < 0 || 2 * (int64_t)qd + 2 > cap) {
        atomicOr(&counts[2], FOHO_SFLEXI_OVER_FACES);
        return;
    }
    const int64_t cube = cid[c];
    FLEXI_IJK(cube, res)
    int64_t q[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        // the flag says the transverse coordinates are in 1 .. res-1: all four cubes exist, and all contain the sign-changing edge
        const int ci = i + c_flexi_ring[axis][r][0], cj = j + c_flexi_ring[axis][r][1], ck = k + c_flexi_ring[axis][r][2];
        const int rk = rank_of(mask, bpre, ((int64_t)ci * res + cj) * res + ck);
        if ((unsigned)rk >= (unsigned)n) return;  // (a mark buffer of another field)
        q[r] = (int64_t)off[rk] + c_flexi_edge_patch[cse[rk]][c_flexi_ring[axis][r][3]];
    }
    flexi_quad(q, cse[c] & 1, faces + 6 * (size_t)qd);  // the edge's near end is corner 0 of this cube
}

// dual vertices (first nvb workgroups, one surface cube per thread) and quads (the rest, one (axis, surface cube) per thread)
__global__ __launch_bounds__(TPB) void k_sf_emit(const float* __restrict__ axes, const float* __restrict__ s, int res,
                                                 const uint64_t* __restrict__ mask, const int32_t* __restrict__ bpre,
                                                 const int32_t* __restrict__ total, int cube_cap, const int32_t* __restrict__ cid,
                                                 const uint8_t* __restrict__ cse, const uint8_t* __restrict__ efl,
                                                 const int32_t* __restrict__ off, const int32_t* __restrict__ gtot, float* __restrict__ verts,
                                                 float* __restrict__ ldev, int verts_cap, int64_t* __restrict__ faces, int faces_cap,
                                                 int32_t* counts, int nvb) {
    const int n = *total;
    if (n <= 0 || n > cube_cap) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = off[n];
        counts[1] = 2 * (*gtot - off[n]);
    }
    if ((int)blockIdx.x < nvb)
        sf_verts_role(gid(), n, axes, s, res, cid, cse, off, verts, ldev, verts_cap, counts);
    else
        sf_faces_role((int64_t)(blockIdx.x - nvb) * TPB + threadIdx.x, n, res, mask, bpre, cid, cse, efl, off, faces, faces_cap, counts);
}

// dL/ds by gather (flexi_core.h: flexi_owns_point, flexi_walk_point): 8 threads per surface cube, one per corner; the owner of a grid
// point P walks its six edges and, on a crossing one, the edge's ring: one term of k_flexi_bwd per (edge, cube), at most 24, summed in
// that order into a register and stored once.  Positions come from the axis tables, so of g . (x_a - x_b) only the edge's own axis is
// left.
__global__ __launch_bounds__(TPB) void k_sf_bwd(const float* __restrict__ axes, const float* __restrict__ s, int res,
                                                const uint64_t* __restrict__ mask, const int32_t* __restrict__ bpre,
                                                const int32_t* __restrict__ total, int cube_cap, const int32_t* __restrict__ cid,
                                                const uint8_t* __restrict__ cse, const int32_t* __restrict__ off,
                                                const float* __restrict__ gverts, int n_verts, float* __restrict__ gs) {
    const int n = usable_count(*total, cube_cap);
    const int64_t t = gid();
    if (t >= 8 * (int64_t)n) return;
    const int64_t cube = cid[t >> 3], C = (int64_t)res * res * res;
    if (cube < 0 || cube >= C) return;
    const int G = res + 1;
    int pt[3];
    if (!flexi_owns_point(cube, (int)(t & 7), res, pt, [&](int64_t c) { return (mask[c >> 6] >> (c & 63)) & 1ull; })) return;
    const size_t gp = flexi_point(pt[0], pt[1], pt[2], G);
    const float sp = s[gp];
    float acc = 0.f, w = 0.f, dx = 0.f;  // w dx: the crossing edge's d crossing / d s_P along its axis
    bool any = false;
    flexi_walk_point(
        pt, res,
        [&](int axis, int side, int mi, int mj, int mk) {
            const float so = s[flexi_point(mi + (side && axis == 0), mj + (side && axis == 1), mk + (side && axis == 2), G)];
            if ((sp < 0.0f) == (so < 0.0f)) return false;
            any = true;
            const float sa = side ? sp : so, sb = side ? so : sp;
            const float D = sb - sa;
            // (s / D) / D as k_flexi_bwd: |s / D| <= 1 on a crossing edge
            w = (side ? sb / D : -sa / D) / D;
            const int m = axis == 0 ? mi : (axis == 1 ? mj : mk);
            dx = axes[axis * G + m] - axes[axis * G + m + 1];
            return true;
        },
        [&](int axis, int, int64_t cc, int e) {
            const int rk = rank_of(mask, bpre, cc);
            if ((unsigned)rk >= (unsigned)n) return;  // (a mark buffer of another field)
            const unsigned code = cse[rk];
            const int p = c_flexi_edge_patch[code][e];
            if (p < 0) return;  // (a workspace of another field)
            const int v = off[rk] + p;
            if ((unsigned)v >= (unsigned)n_verts) return;
            acc += (gverts[3 * (size_t)v + axis] / flexi_patch_edges(code, p)) * dx * w;
        });
    if (any) gs[gp] = acc;
}

bool res_ok(int32_t r) { return r >= 1 && r <= FOHO_SFLEXI_MAX_RES; }
bool cap_ok(int32_t c) { return c >= 0 && c <= FOHO_SFLEXI_MAX_CUBES; }

}  // namespace

FOHO_SIDE_ENTRY_POINTS(sflexi, FOHO_SFLEXI_API, FOHO_SFLEXI_VERSION)

extern "C" {

FOHO_SFLEXI_API size_t foho_sflexi_mark_bytes(int32_t res) { return res_ok(res) ? carve_mark(nullptr, res).bytes : 0; }

FOHO_SFLEXI_API size_t foho_sflexi_cube_bytes(int32_t cube_cap) { return cap_ok(cube_cap) ? carve_cube(nullptr, cube_cap).bytes : 0; }

FOHO_SFLEXI_API size_t foho_sflexi_workspace_bytes(int32_t res, int32_t cube_cap) {
    if (!res_ok(res) || !cap_ok(cube_cap)) return 0;
    return carve_mark(nullptr, res).bytes + carve_cube(nullptr, cube_cap).bytes;
}

FOHO_SFLEXI_API int foho_sflexi_mark(const float* s, int32_t res, void* marks, size_t marks_bytes, int32_t* n_cubes, void* stream) {
    if (!s || !marks || !n_cubes) return fail(-1, "foho_sflexi_mark: null argument");
    if (!res_ok(res)) return fail(-1, "foho_sflexi_mark: resolution outside 1 .. 1024");
    const MarkWs w = carve_mark(marks, res);
    if (marks_bytes < w.bytes) return fail(-3, "foho_sflexi_mark: mark buffer too small (query foho_sflexi_mark_bytes)");
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sf_mark, dim3((unsigned)w.blocks), dim3(TPB), 0, st, s, res, w.mask, w.bpre);
    Seq q{};
    q.i32 = w.bpre, q.n_host = (int64_t)w.blocks;
    hipLaunchKernelGGL(k_sf_sums, dim3((unsigned)w.chunks), dim3(TPB), 0, st, q, w.csum);
    hipLaunchKernelGGL(k_sf_scan_chunks, dim3(1), dim3(TPB), 0, st, q, w.csum);
    hipLaunchKernelGGL(k_sf_apply, dim3((unsigned)w.chunks), dim3(TPB), 0, st, q, w.csum, w.bpre, w.total, n_cubes);
    return launched("foho_sflexi_mark");
}

FOHO_SFLEXI_API int foho_sflexi_extract(const float* axes, const float* s, int32_t res, const void* marks, size_t marks_bytes,
                                        int32_t cube_cap, float* verts, int32_t verts_cap, int64_t* faces, int32_t faces_cap,
                                        float* l_dev, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (!axes || !s || !marks || !verts || !faces || !counts || !workspace) return fail(-1, "foho_sflexi_extract: null argument");
    if (!res_ok(res)) return fail(-1, "foho_sflexi_extract: resolution outside 1 .. 1024");
    if (!cap_ok(cube_cap) || verts_cap < 0 || faces_cap < 0) return fail(-1, "foho_sflexi_extract: bad capacity");
    const MarkWs m = carve_mark(marks, res);
    if (marks_bytes < m.bytes) return fail(-3, "foho_sflexi_extract: mark buffer too small (query foho_sflexi_mark_bytes)");
    const CubeWs w = carve_cube(workspace, cube_cap);
    if (workspace_bytes < w.bytes) return fail(-3, "foho_sflexi_extract: workspace too small (query foho_sflexi_cube_bytes)");
    const hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)cube_cap;
    hipLaunchKernelGGL(k_sf_compact, dim3(blocks_for(m.words, TPB)), dim3(TPB), 0, st, m.mask, m.bpre, m.total, (int64_t)m.words, cube_cap, w.cid,
                       counts);
    hipLaunchKernelGGL(k_sf_classify, dim3(blocks_for(n, TPB)), dim3(TPB), 0, st, s, res, m.total, cube_cap, w.cid, w.cse, w.efl);
    Seq q{};
    q.cse = w.cse, q.efl = w.efl, q.n_dev = m.total, q.cap = cube_cap;
    hipLaunchKernelGGL(k_sf_sums, dim3(blocks_for(w.chunks, 1)), dim3(TPB), 0, st, q, w.csum);
    hipLaunchKernelGGL(k_sf_scan_chunks, dim3(1), dim3(TPB), 0, st, q, w.csum);
    hipLaunchKernelGGL(k_sf_apply, dim3(blocks_for(w.chunks, 1)), dim3(TPB), 0, st, q, w.csum, w.off, w.gtot, (int32_t*)nullptr);
    const int nvb = (int)blocks_for(n, TPB);
    hipLaunchKernelGGL(k_sf_emit, dim3(nvb + blocks_for(3 * n, TPB)), dim3(TPB), 0, st, axes, s, res, m.mask, m.bpre, m.total, cube_cap, w.cid,
                       w.cse, w.efl, w.off, w.gtot, verts, l_dev, verts_cap, faces, faces_cap, counts, nvb);
    return launched("foho_sflexi_extract");
}

FOHO_SFLEXI_API int foho_sflexi_bwd(const float* axes, const float* s, int32_t res, const void* marks, size_t marks_bytes,
                                    int32_t cube_cap, const float* grad_verts, int32_t n_verts, float* grad_s, const void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (!axes || !s || !marks || !grad_verts || !grad_s || !workspace) return fail(-1, "foho_sflexi_bwd: null argument");
    if (!res_ok(res)) return fail(-1, "foho_sflexi_bwd: resolution outside 1 .. 1024");
    if (!cap_ok(cube_cap)) return fail(-1, "foho_sflexi_bwd: bad capacity");
    if (n_verts < 0) return fail(-1, "foho_sflexi_bwd: negative vertex count");
    const MarkWs m = carve_mark(marks, res);
    if (marks_bytes < m.bytes) return fail(-3, "foho_sflexi_bwd: mark buffer too small (query foho_sflexi_mark_bytes)");
    const CubeWs w = carve_cube(const_cast<void*>(workspace), cube_cap);
    if (workspace_bytes < w.bytes) return fail(-3, "foho_sflexi_bwd: workspace too small (query foho_sflexi_cube_bytes)");
    if (cube_cap == 0 || n_verts == 0) return 0;
    hipLaunchKernelGGL(k_sf_bwd, dim3(blocks_for(8 * (size_t)cube_cap, TPB)), dim3(TPB), 0, (hipStream_t)stream, axes, s, res, m.mask, m.bpre,
                       m.total, cube_cap, w.cid, w.cse, w.off, grad_verts, n_verts, grad_s);
    return launched("foho_sflexi_bwd");
}

}  // extern "C"
