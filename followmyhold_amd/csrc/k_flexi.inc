// k_flexi.inc -- differentiable iso-surfacing of the object's SDF grid: FlexiCubes with default weights = Dual Marching
// Cubes (kaolin FlexiCubes.__call__ as called at pipelines.py:1393 / 1509; SURVEY.md 8(f) rank 1).
//
//   k_flexi_classify   per cube: inside/outside code of its 8 corners + number of dual vertices (patch table);
//                      per grid edge: 1 when it changes sign and all four cubes around it exist
//   scan (2 kernels)   exclusive prefix sums -> vertex offset of every cube, quad offset of every edge (deterministic
//                      output order: vertices by (cube, patch), faces by (axis, i, j, k) of their edge); both arrays per launch
//   k_flexi_emit       dual vertices and quads in one launch:
//     vertices         per surface cube: zero crossings u_e = (x_a s_b - x_b s_a) / (s_b - s_a), dual vertex = mean of the
//                      crossings of a patch, L_dev = mean absolute deviation of the crossing distances
//     faces            per sign-change edge: quad through the dual vertices of its four cubes, oriented inside -> outside,
//                      split along its first diagonal
//   k_flexi_bwd        d(vertices)/d(sdf, grid positions) scattered with float atomics
//
// Grid point (i,j,k) -> (i*G + j)*G + k (generate_dense_grid_points, PL:341-360); cube corners in x-fastest order; cube edges
// 0-3 along x, 4-7 along y, 8-11 along z (followmyhold_amd/flexi_tables.py).
// The per-cube arithmetic (index helpers, sign code, dual vertex and l_dev, patch edge count, ring table, quad orientation and split) is
// flexi_core.h's, shared with the sparse extractor (foho_sflexi.hip) and the weighted one (foho_wflexi.hip).  The four scan kernels
// are three device functions (scan_load8, scan_block_sum, scan_store8) around their own choice of array and prefix.
#include "flexi_core.h"

constexpr int FX_ITEMS = 2048;  // items per workgroup of the scan (256 threads x 8)

struct FlexiWs {
    uint8_t* cse;
    int32_t *npatch, *v_off, *ecross, *f_off, *bsum_v, *bsum_f;
    size_t total;
};
static FlexiWs carve_flexi(void* ws, int res) {
    const size_t G = (size_t)res + 1, C = (size_t)res * res * res, E = 3 * G * G * G;
    const size_t nbv = (C + FX_ITEMS - 1) / FX_ITEMS, nbf = (E + FX_ITEMS - 1) / FX_ITEMS;
    char* p = (char*)ws;
    Carve cv;
    FlexiWs w;
    w.cse = (uint8_t*)(p + cv.take(C));
    w.npatch = (int32_t*)(p + cv.take(C * 4));
    w.v_off = (int32_t*)(p + cv.take(C * 4));
    w.ecross = (int32_t*)(p + cv.take(E * 4));
    w.f_off = (int32_t*)(p + cv.take(E * 4));
    w.bsum_v = (int32_t*)(p + cv.take((nbv + 1) * 4));
    w.bsum_f = (int32_t*)(p + cv.take((nbf + 1) * 4));
    w.total = cv.off;
    return w;
}

extern "C" size_t foho_flexi_workspace_bytes(int32_t res) {
    if (res < 1 || res > 1024) return 0;
    return carve_flexi(nullptr, res).total;
}

__global__ __launch_bounds__(256) void k_flexi_classify(const float* s, int res, uint8_t* cse, int32_t* npatch, int32_t* ecross) {
    const int G = res + 1;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t C = (size_t)res * res * res, G3 = (size_t)G * G * G;
    if (t < C) {
        FLEXI_IJK(t, res)
        const unsigned code = flexi_cube_code(s, res, i, j, k);
        cse[t] = (uint8_t)code;
        npatch[t] = c_flexi_npatch[code];
    }
    if (t < 3 * G3) {
        const int axis = (int)(t / G3);
        const size_t r = t % G3;
        FLEXI_IJK(r, G)
        const int di = axis == 0, dj = axis == 1, dk = axis == 2;
        int flag = 0;
        // the edge exists when its far end is a grid point; it has four cubes when the two transverse coordinates are interior
        const bool along = (di ? i : (dj ? j : k)) < res;
        const bool t1 = di ? (j >= 1 && j <= res - 1) : (i >= 1 && i <= res - 1);
        const bool t2 = dk ? (j >= 1 && j <= res - 1) : (k >= 1 && k <= res - 1);
        if (along && t1 && t2) {
            // (flexi_point written out: through the call the compiler orders this kernel's instructions differently)
            const float sa = s[r], sb = s[((size_t)(i + di) * G + (j + dj)) * G + (k + dk)];
            flag = ((sa < 0.0f) != (sb < 0.0f)) ? 1 : 0;
        }
        ecross[t] = flag;
    }
}

// ---- exclusive scan of an int32 array (two launches: block sums, then every workgroup adds up the sums in front of it; deterministic).  A workgroup takes FX_ITEMS items, 8 in a row per thread.
// The three pieces of its kernels; s_w = 4 ints of LDS:
// my 8 items of `in` (0 past n) -> v; their sum
__device__ __forceinline__ int scan_load8(const int32_t* in, size_t base, size_t n, int* v) {
    int sum = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        v[q] = (base + q < n) ? in[base + q] : 0;
        sum += v[q];
    }
    return sum;
}
// the sum of the workgroup's items (one barrier)
__device__ __forceinline__ int scan_block_sum(const int32_t* in, size_t base, size_t n, int* s_w) {
    int v = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) v += (base + q < n) ? in[base + q] : 0;
    const unsigned w = wave_sum((unsigned)v);
    if (lane_id() == 0) s_w[wave_id()] = (int)w;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}
// the exclusive prefixes of my 8 items -> out, given the total in front of the workgroup (one barrier); the running total behind my
// last item
__device__ __forceinline__ int scan_store8(const int* v, int sum, int prefix, size_t base, size_t n, int32_t* out, int* s_w) {
    const unsigned incl = wave_incl_scan((unsigned)sum);
    if (lane_id() == 63) s_w[wave_id()] = (int)incl;
    __syncthreads();
    int off = prefix + (int)incl - sum;
    for (int w = 0; w < wave_id(); w++) off += s_w[w];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        if (base + q < n) out[base + q] = off;
        off += v[q];
    }
    return off;
}

__global__ __launch_bounds__(256) void k_scan_sums(const int32_t* in, size_t n, int32_t* bsum) {
    __shared__ int s_w[4];
    const int sum = scan_block_sum(in, (size_t)blockIdx.x * FX_ITEMS + (size_t)threadIdx.x * 8, n, s_w);
    if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
}

// the two scans of the extraction (dual vertices per cube, quads per grid edge) ride in the same two launches
struct Scan2 {
    const int32_t* in[2];
    size_t n[2];
    int32_t* bsum[2];
    int32_t* out[2];
    int nb[2];
};
__global__ __launch_bounds__(256) void k_scan2_sums(Scan2 a) {
    __shared__ int s_w[4];
    const int which = ((int)blockIdx.x < a.nb[0]) ? 0 : 1;
    const int blk = which ? blockIdx.x - a.nb[0] : blockIdx.x;
    const int sum = scan_block_sum(which ? a.in[1] : a.in[0], (size_t)blk * FX_ITEMS + (size_t)threadIdx.x * 8, which ? a.n[1] : a.n[0], s_w);
    if (threadIdx.x == 0) (which ? a.bsum[1] : a.bsum[0])[blk] = sum;
}
// exclusive prefix of the block sums in front of workgroup `blk`, computed by the workgroup itself (at most a few hundred
// values: cheaper than a launch for a serial scan of them).  Whole workgroup; s_w = 4 ints of LDS.  Ends with a barrier.
__device__ __forceinline__ int block_prefix(const int32_t* bsum, int blk, int* s_w) {
    int v = 0;
    for (int i = threadIdx.x; i < blk; i += 256) v += bsum[i];
    const unsigned w = wave_sum((unsigned)v);
    __syncthreads();
    if (lane_id() == 0) s_w[wave_id()] = (int)w;
    __syncthreads();
    const int r = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    __syncthreads();
    return r;
}
// counts (optional) = [total of array 0, 2 * total of array 1, 0], written by the last workgroup of each array
__global__ __launch_bounds__(256) void k_scan2_apply(Scan2 a, int32_t* counts) {
    __shared__ int s_w[4];
    const int which = ((int)blockIdx.x < a.nb[0]) ? 0 : 1;
    const int blk = which ? blockIdx.x - a.nb[0] : blockIdx.x;
    const int32_t* in = which ? a.in[1] : a.in[0];
    const int32_t* bsum = which ? a.bsum[1] : a.bsum[0];
    int32_t* out = which ? a.out[1] : a.out[0];
    const size_t n = which ? a.n[1] : a.n[0];
    const size_t base = (size_t)blk * FX_ITEMS + (size_t)threadIdx.x * 8;
    int v[8];
    const int sum = scan_load8(in, base, n, v);
    const int prefix = block_prefix(bsum, blk, s_w);
    const int off = scan_store8(v, sum, prefix, base, n, out, s_w);
    if (counts && blk == (which ? a.nb[1] : a.nb[0]) - 1 && threadIdx.x == 255) {  // off = grand total after the last item
        if (which == 0) {
            counts[0] = off;
            counts[2] = 0;
        } else {
            counts[1] = 2 * off;
        }
    }
}
// single array, same scheme (both topology-table builders: k_topo.inc's topo_scan)
__global__ __launch_bounds__(256) void k_scan_apply_p(const int32_t* in, size_t n, const int32_t* bsum, int32_t* out) {
    __shared__ int s_w[4];
    const size_t base = (size_t)blockIdx.x * FX_ITEMS + (size_t)threadIdx.x * 8;
    int v[8];
    const int sum = scan_load8(in, base, n, v);
    const int prefix = block_prefix(bsum, (int)blockIdx.x, s_w);
    scan_store8(v, sum, prefix, base, n, out, s_w);
}

__device__ __forceinline__ void flexi_corners(const float* x, const float* s, int res, size_t t, float* sc, float* xc) {
    const int G = res + 1;
    FLEXI_IJK(t, res)
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const size_t gi = flexi_corner(i, j, k, c, G);
        sc[c] = s[gi];
        for (int q = 0; q < 3; q++) xc[3 * c + q] = x[3 * gi + q];
    }
}

// counts: [0] vertices, [1] triangles, [2] overflow flags (bit0 vertex capacity, bit1 face capacity)
__device__ __forceinline__ void flexi_verts_role(size_t t, const float* x, const float* s, int res, const uint8_t* cse, const int32_t* npatch,
                                                 const int32_t* v_off, float* verts, float* ldev, int cap, int32_t* counts) {
    if (t >= (size_t)res * res * res) return;
    const int np = npatch[t];
    if (np == 0) return;
    const int base = v_off[t];
    if (base + np > cap) {
        atomicOr(&counts[2], 1);
        return;
    }
    const unsigned code = cse[t];
    float sc[8], xc[24];
    flexi_corners(x, s, res, t, sc, xc);
    for (int p = 0; p < np; p++) flexi_dual_vertex(code, p, sc, xc, verts + 3 * (size_t)(base + p), ldev ? ldev + (base + p) : nullptr);
}

__device__ __forceinline__ void flexi_faces_role(size_t t, const float* s, int res, const uint8_t* cse, const int32_t* v_off,
                                                 const int32_t* ecross, const int32_t* f_off, int64_t* faces, int cap, int32_t* counts) {
    const int G = res + 1;
    const size_t G3 = (size_t)G * G * G;
    if (t >= 3 * G3 || !ecross[t]) return;
    const int qd = f_off[t];
    if (2 * qd + 2 > cap) {
        atomicOr(&counts[2], 2);
        return;
    }
    const int axis = (int)(t / G3);
    const size_t r = t % G3;
    FLEXI_IJK(r, G)
    int64_t q[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int ci = i + c_flexi_ring[axis][c][0], cj = j + c_flexi_ring[axis][c][1], ck = k + c_flexi_ring[axis][c][2];
        const size_t cid = ((size_t)ci * res + cj) * res + ck;
        q[c] = (int64_t)v_off[cid] + c_flexi_edge_patch[cse[cid]][c_flexi_ring[axis][c][3]];
    }
    flexi_quad(q, s[r] < 0.0f, faces + 6 * (size_t)qd);  // the edge's near end is grid point r
}

// dual vertices (first nvb workgroups, one cube per thread) and quads (the rest, one grid edge per thread) in one launch
__global__ __launch_bounds__(256) void k_flexi_emit(const float* x, const float* s, int res, const uint8_t* cse, const int32_t* npatch,
                                                    const int32_t* v_off, const int32_t* ecross, const int32_t* f_off, float* verts,
                                                    float* ldev, int verts_cap, int64_t* faces, int faces_cap, int32_t* counts, int nvb) {
    if ((int)blockIdx.x < nvb)
        flexi_verts_role((size_t)blockIdx.x * 256 + threadIdx.x, x, s, res, cse, npatch, v_off, verts, ldev, verts_cap, counts);
    else
        flexi_faces_role((size_t)(blockIdx.x - nvb) * 256 + threadIdx.x, s, res, cse, v_off, ecross, f_off, faces, faces_cap, counts);
}

extern "C" int foho_flexi_fwd(const float* x, const float* s, int32_t res, float* verts, int32_t verts_cap, int64_t* faces,
                              int32_t faces_cap, float* l_dev, int32_t* counts, void* workspace, size_t workspace_bytes,
                              void* stream_) {
    if (!x || !s || !verts || !faces || !counts || res < 1 || res > 1024 || verts_cap < 0 || faces_cap < 0) {
        foho_set_error("foho_flexi_fwd: bad argument");
        return FOHO_ERR_BAD_ARG;
    }
    const FlexiWs w = carve_flexi(workspace, res);
    if (!workspace || workspace_bytes < w.total) {
        foho_set_error("foho_flexi_fwd: workspace too small (query foho_flexi_workspace_bytes)");
        return FOHO_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const size_t G = (size_t)res + 1, C = (size_t)res * res * res, E = 3 * G * G * G;
    const int nbv = (int)((C + FX_ITEMS - 1) / FX_ITEMS), nbf = (int)((E + FX_ITEMS - 1) / FX_ITEMS);
    hipLaunchKernelGGL(k_flexi_classify, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream, s, res, w.cse, w.npatch, w.ecross);
    CHECK_LAUNCH("k_flexi_classify");
    Scan2 sc;
    sc.in[0] = w.npatch, sc.in[1] = w.ecross;
    sc.n[0] = C, sc.n[1] = E;
    sc.bsum[0] = w.bsum_v, sc.bsum[1] = w.bsum_f;
    sc.out[0] = w.v_off, sc.out[1] = w.f_off;
    sc.nb[0] = nbv, sc.nb[1] = nbf;
    hipLaunchKernelGGL(k_scan2_sums, dim3(nbv + nbf), dim3(256), 0, stream, sc);
    CHECK_LAUNCH("k_scan2_sums");
    hipLaunchKernelGGL(k_scan2_apply, dim3(nbv + nbf), dim3(256), 0, stream, sc, counts);
    CHECK_LAUNCH("k_scan2_apply");
    const int nvb = (int)((C + 255) / 256);
    hipLaunchKernelGGL(k_flexi_emit, dim3((unsigned)(nvb + (E + 255) / 256)), dim3(256), 0, stream, x, s, res, w.cse, w.npatch, w.v_off,
                       w.ecross, w.f_off, verts, l_dev, verts_cap, faces, faces_cap, counts, nvb);
    CHECK_LAUNCH("k_flexi_emit");
    return FOHO_OK;
}

// d(vertices) / d(sdf, grid positions): u = (x_a s_b - x_b s_a) / D, D = s_b - s_a;
// du/ds_a = s_b (x_a - x_b) / D^2, du/ds_b = -s_a (x_a - x_b) / D^2, du/dx_a = s_b / D, du/dx_b = -s_a / D
__global__ __launch_bounds__(256) void k_flexi_bwd(const float* x, const float* s, int res, const uint8_t* cse, const int32_t* npatch,
                                                   const int32_t* v_off, const float* gverts, int n_verts, float* gs, float* gx) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)res * res * res) return;
    const int np = npatch[t];
    if (np == 0) return;
    const int base = v_off[t];
    if (base + np > n_verts) return;
    const int G = res + 1;
    FLEXI_IJK(t, res)
    FLEXI_EDGE_TABLES
    const unsigned code = cse[t];
    float sc[8], xc[24];
    flexi_corners(x, s, res, t, sc, xc);
    for (int p = 0; p < np; p++) {
        const float cnt = flexi_patch_edges(code, p);
        float g[3];
        for (int q = 0; q < 3; q++) g[q] = gverts[3 * (size_t)(base + p) + q] / cnt;
#pragma unroll
        for (int e = 0; e < 12; e++) {
            if (c_flexi_edge_patch[code][e] != p) continue;
            const int a = fx_ea[e], b = fx_eb[e];
            const size_t ga = flexi_corner(i, j, k, a, G), gb = flexi_corner(i, j, k, b, G);
            const float D = sc[b] - sc[a];
            float dot = 0.f;
            for (int q = 0; q < 3; q++) dot += g[q] * (xc[3 * a + q] - xc[3 * b + q]);
            // 1 / D^2 as two divisions: D * D underflows for |D| < 1e-19 while |s / D| <= 1 on a crossing edge, so (s / D) / D
            // overflows only where the gradient itself does
            const float wa = sc[b] / D, wb = -sc[a] / D;
            atomicAdd(&gs[ga], dot * (wa / D));
            atomicAdd(&gs[gb], dot * (wb / D));
            if (gx) {
                for (int q = 0; q < 3; q++) {
                    atomicAdd(&gx[3 * ga + q], g[q] * wa);
                    atomicAdd(&gx[3 * gb + q], g[q] * wb);
                }
            }
        }
    }
}

extern "C" int foho_flexi_bwd(const float* x, const float* s, int32_t res, const float* grad_verts, int32_t n_verts, float* grad_s,
                              float* grad_x, const void* workspace, size_t workspace_bytes, void* stream_) {
    if (!x || !s || !grad_verts || !grad_s || res < 1 || res > 1024 || n_verts < 0) {
        foho_set_error("foho_flexi_bwd: bad argument");
        return FOHO_ERR_BAD_ARG;
    }
    const FlexiWs w = carve_flexi(const_cast<void*>(workspace), res);
    if (!workspace || workspace_bytes < w.total) {
        foho_set_error("foho_flexi_bwd: workspace too small");
        return FOHO_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const size_t C = (size_t)res * res * res;
    hipLaunchKernelGGL(k_flexi_bwd, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, x, s, res, w.cse, w.npatch, w.v_off, grad_verts,
                       n_verts, grad_s, grad_x);
    CHECK_LAUNCH("k_flexi_bwd");
    return FOHO_OK;
}
