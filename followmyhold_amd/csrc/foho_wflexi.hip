// foho_wflexi.hip -- libfoho_wflexi.so: FlexiCubes with alpha, beta, gamma and the training-mode triangulation, forward and gradient
// (foho_wflexi.h: semantics and orderings; weighted_flexi.py).
//
//   k_wf_classify   one thread per cube: sign code and the three quad-owning flags of the grid edges at its minimum corner
//                   (k_sf_classify's rule) -> one uint16 per cube; per block of 256 cubes the counts (surface cubes, dual vertices,
//                   quads of axis 0, 1, 2)
//   k_wf_blocks     one workgroup: exclusive scan of the block counts, the totals
//   k_wf_offsets    one thread per cube: the scan inside the block -> rank of a surface cube (dense, int32) and, by rank, its id, its
//                   vertex offset and its three quad indices; the counts
//   k_wf_verts      per surface cube: dual vertices and l_dev (flexi_dual_vertex with the weights)
//   k_wf_faces      per (surface cube, axis): the quad of the owned edge, ids and gammas oriented by flexi_orient; flexi_split along
//                   the diagonal gamma chooses, or the centre and four triangles.  A launch of its own because the centre reads the
//                   four dual vertices
//   k_wf_bwd_cube   per surface cube: dL/dalpha and dL/dbeta rows, dL/dgamma and the centres' gradient to its dual vertices by a walk
//                   over the quads of its twelve edges, and one float4 record (dL/ds, dL/dx) per (edge, end); the forward's
//                   quantities come from one call of flexi_dual_vertex per patch
//   k_wf_bwd_gather 8 threads per surface cube: the owner of a grid point sums its at most 24 records and stores once (flexi_core.h's
//                   ownership rule and walk, k_sf_bwd's)
// Everything behind k_wf_offsets works on the list of surface cubes.  STRICT flags (-ffp-contract=off, correctly rounded division and
// sqrt), as foho_sflexi.hip, and the per-cube arithmetic is flexi_core.h's, the one the dense and sparse extractors call without
// weights: with unit weights the vertices, l_dev and faces are bitwise foho_flexi_fwd's.  What is written here is the list of surface
// cubes, the weight rows, the centres of training mode and the backward's own terms.
#include "flexi_core.h"
#include "foho_carve.h"
#include "foho_side.h"
#include "foho_wflexi.h"

namespace {

// surface cubes, dual vertices, quads per axis: scanned together
struct Cnt5 {
    int v[5];
    Cnt5() = default;
    __host__ __device__ Cnt5(int z) {
        for (int i = 0; i < 5; i++) v[i] = z;
    }
    __device__ Cnt5& operator+=(const Cnt5& o) {
        for (int i = 0; i < 5; i++) v[i] += o.v[i];
        return *this;
    }
    __device__ Cnt5 operator+(const Cnt5& o) const {
        Cnt5 r = *this;
        r += o;
        return r;
    }
    __device__ Cnt5 operator-(const Cnt5& o) const {
        Cnt5 r;
        for (int i = 0; i < 5; i++) r.v[i] = v[i] - o.v[i];
        return r;
    }
};

struct Ws {
    uint16_t* info;  // C: sign code | owner flags << 8
    int32_t* rank;   // C: index of a surface cube in the list (written for surface cubes only)
    Cnt5 *bcnt, *bpre;
    int32_t* tot;  // surface cubes, dual vertices, quads of axis 0, 1, 2
    int32_t *cid, *voff, *qoff;  // cap, cap, 3 cap: by rank; qoff < 0 where the edge owns no quad
    size_t blocks, bytes;
};
Ws carve(const void* ws, int res, int cap) {
    const size_t C = (size_t)res * res * res, n = (size_t)cap;
    Ws w;
    w.blocks = (C + TPB - 1) / TPB;
    char* p = (char*)const_cast<void*>(ws);
    Carve cv;
    w.info = (uint16_t*)(p + cv.take(C * 2));
    w.rank = (int32_t*)(p + cv.take(C * 4));
    w.bcnt = (Cnt5*)(p + cv.take(w.blocks * sizeof(Cnt5)));
    w.bpre = (Cnt5*)(p + cv.take(w.blocks * sizeof(Cnt5)));
    w.tot = (int32_t*)(p + cv.take(5 * 4));
    w.cid = (int32_t*)(p + cv.take(n * 4));
    w.voff = (int32_t*)(p + cv.take(n * 4));
    w.qoff = (int32_t*)(p + cv.take(3 * n * 4));
    w.bytes = cv.off;
    return w;
}

__device__ __forceinline__ Cnt5 cube_counts(unsigned info) {
    const unsigned code = info & 255u;
    Cnt5 c;
    c.v[0] = (code != 0u && code != 255u) ? 1 : 0;
    c.v[1] = c_flexi_npatch[code];
    for (int a = 0; a < 3; a++) c.v[2 + a] = (info >> (8 + a)) & 1u;
    return c;
}

__global__ __launch_bounds__(TPB) void k_wf_classify(const float* __restrict__ s, int res, uint16_t* __restrict__ info,
                                                     Cnt5* __restrict__ bcnt) {
    __shared__ Cnt5 sh[TPB];
    __shared__ Cnt5 tot;
    const int64_t p = gid(), C = (int64_t)res * res * res;
    unsigned v = 0;
    if (p < C) {
        FLEXI_IJK(p, res)
        const unsigned code = flexi_cube_code(s, res, i, j, k);
        // the edge from the minimum corner along an axis has four cubes around it when its two transverse coordinates are interior; its
        // ends are corners 0 and 1 / 2 / 4
        const bool ii = i >= 1 && i <= res - 1, jj = j >= 1 && j <= res - 1, kk = k >= 1 && k <= res - 1;
        unsigned f = 0;
        if (jj && kk) f |= (code ^ (code >> 1)) & 1u;
        if (ii && kk) f |= ((code ^ (code >> 2)) & 1u) << 1;
        if (ii && jj) f |= ((code ^ (code >> 4)) & 1u) << 2;
        v = code | (f << 8);
        info[p] = (uint16_t)v;
    }
    block_exclusive_scan<TPB>(cube_counts(v), sh, &tot);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(TPB) void k_wf_blocks(const Cnt5* __restrict__ bcnt, int nb, Cnt5* __restrict__ bpre, int32_t* __restrict__ total) {
    __shared__ Cnt5 sh[TPB];
    __shared__ Cnt5 tot;
    Cnt5 carry(0);
    for (int base = 0; base < nb; base += TPB) {
        const int i = base + (int)threadIdx.x;
        const Cnt5 v = i < nb ? bcnt[i] : Cnt5(0);
        const Cnt5 ex = block_exclusive_scan<TPB>(v, sh, &tot);
        if (i < nb) bpre[i] = carry + ex;
        carry += tot;
        __syncthreads();  // tot is read before the next round's scan writes it
    }
    if (threadIdx.x == 0)
        for (int q = 0; q < 5; q++) total[q] = carry.v[q];
}

__global__ __launch_bounds__(TPB) void k_wf_offsets(const uint16_t* __restrict__ info, int res, const Cnt5* __restrict__ bpre,
                                                    const int32_t* __restrict__ total, int cap, int training, int32_t* __restrict__ rank,
                                                    int32_t* __restrict__ cid, int32_t* __restrict__ voff, int32_t* __restrict__ qoff,
                                                    int32_t* __restrict__ counts) {
    __shared__ Cnt5 sh[TPB];
    const int64_t p = gid(), C = (int64_t)res * res * res;
    const int n = total[0], V = total[1], Q = total[2] + total[3] + total[4];
    if (p == 0) {
        counts[0] = V;
        counts[1] = training ? V + Q : V;
        counts[2] = training ? 4 * Q : 2 * Q;
        counts[3] = n > cap ? FOHO_WFLEXI_OVER_VERTS : 0;  // a surface cube has at least one vertex: V >= n > verts_cap
        counts[4] = n;
    }
    const unsigned v = p < C ? info[p] : 0u;
    const Cnt5 mine = cube_counts(v);
    const Cnt5 ex = block_exclusive_scan<TPB>(mine, sh);
    if (!mine.v[0]) return;
    const Cnt5 o = bpre[blockIdx.x] + ex;
    const int r = o.v[0];
    rank[p] = r;
    if (r >= cap) return;
    cid[r] = (int32_t)p;
    voff[r] = o.v[1];
    int axis_base = 0;
    for (int a = 0; a < 3; a++) {
        qoff[3 * (size_t)r + a] = mine.v[2 + a] ? axis_base + o.v[2 + a] : -1;
        axis_base += total[2 + a];
    }
}

// corner values, corner positions and the cube's rows of alpha and beta (1 where the weight is not given).  The corner part is
// k_flexi.inc's flexi_corners with the alpha row between its loads: split in two calls, k_wf_verts takes four registers more and
// loses a wave of occupancy
__device__ __forceinline__ void load_cube(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ alpha,
                                          const float* __restrict__ beta, int res, int64_t cube, float* sc, float* xc, float* al, float* be) {
    const int G = res + 1;
    FLEXI_IJK(cube, res)
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const size_t gi = flexi_corner(i, j, k, c, G);
        sc[c] = s[gi];
        for (int q = 0; q < 3; q++) xc[3 * c + q] = x[3 * gi + q];
        al[c] = alpha ? alpha[8 * (size_t)cube + c] : 1.0f;
    }
#pragma unroll
    for (int e = 0; e < 12; e++) be[e] = beta ? beta[12 * (size_t)cube + e] : 1.0f;
}

__global__ __launch_bounds__(TPB) void k_wf_verts(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ alpha,
                                                  const float* __restrict__ beta, int res, const uint16_t* __restrict__ info,
                                                  const int32_t* __restrict__ total, int cap, const int32_t* __restrict__ cid,
                                                  const int32_t* __restrict__ voff, float* __restrict__ verts, float* __restrict__ ldev,
                                                  int32_t* counts) {
    const int64_t t = gid();
    if (t >= usable_count(total[0], cap)) return;
    const int64_t cube = cid[t];
    if (cube < 0 || cube >= (int64_t)res * res * res) return;  // (a workspace of another resolution)
    const unsigned code = info[cube] & 255u;
    const int np = c_flexi_npatch[code], base = voff[t];
    if (base < 0 || base + np > cap) {
        atomicOr(&counts[3], FOHO_WFLEXI_OVER_VERTS);
        return;
    }
    float sc[8], xc[24], al[8], be[12];
    load_cube(x, s, alpha, beta, res, cube, sc, xc, al, be);
    for (int p = 0; p < np; p++) flexi_dual_vertex(code, p, sc, xc, al, be, verts + 3 * (size_t)(base + p), ldev ? ldev + (base + p) : nullptr);
}

// the ring of the axis-`axis` edge that starts at grid point (i,j,k), all four cubes in the grid: their ids and ranks
__device__ __forceinline__ bool ring_of(int axis, int i, int j, int k, int res, const int32_t* __restrict__ rank, int n, int64_t* cc, int* rk) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int ci = i + c_flexi_ring[axis][r][0], cj = j + c_flexi_ring[axis][r][1], ck = k + c_flexi_ring[axis][r][2];
        cc[r] = ((int64_t)ci * res + cj) * res + ck;
        rk[r] = rank[cc[r]];  // surface cubes all: each contains the sign-changing edge
        if ((unsigned)rk[r] >= (unsigned)n) return false;
    }
    return true;
}

__global__ __launch_bounds__(TPB) void k_wf_faces(const float* __restrict__ gamma, int res, int training, const uint16_t* __restrict__ info,
                                                  const int32_t* __restrict__ rank, const int32_t* __restrict__ total, int cap,
                                                  const int32_t* __restrict__ cid, const int32_t* __restrict__ voff,
                                                  const int32_t* __restrict__ qoff, float* __restrict__ verts, int64_t* __restrict__ faces,
                                                  int faces_cap, int32_t* counts) {
    const int64_t t = gid();
    const int n = usable_count(total[0], cap);
    if (t >= 3 * (int64_t)n) return;
    const int axis = (int)(t % 3);
    const int64_t c = t / 3;
    const int qd = qoff[t];
    if (qd < 0) return;
    const int V = total[1], per = training ? 4 : 2;
    if ((int64_t)per * qd + per > faces_cap) {
        atomicOr(&counts[3], FOHO_WFLEXI_OVER_FACES);
        return;
    }
    if (V > cap || (training && (int64_t)V + qd + 1 > cap)) {
        atomicOr(&counts[3], FOHO_WFLEXI_OVER_VERTS);
        return;
    }
    const int64_t cube = cid[c];
    if (cube < 0 || cube >= (int64_t)res * res * res) return;
    FLEXI_IJK(cube, res)
    int64_t cc[4], q[4];
    int rk[4];
    if (!ring_of(axis, i, j, k, res, rank, n, cc, rk)) return;
    float g[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        q[r] = (int64_t)voff[rk[r]] + c_flexi_edge_patch[info[cc[r]] & 255u][c_flexi_ring[axis][r][3]];
        g[r] = gamma ? gamma[cc[r]] : 1.0f;
    }
    const bool near_inside = info[cube] & 1u;  // the edge's near end is corner 0 of this cube
    flexi_orient(q, near_inside);
    flexi_orient(g, near_inside);
    int64_t* out = faces + 3 * (size_t)per * qd;
    if (!training) {
        flexi_split(q, g[1] * g[3] > g[0] * g[2], out);  // the second diagonal only where its product is strictly larger
        return;
    }
    const float g02 = g[0] * g[2], g13 = g[1] * g[3], den = (g02 + g13) + 1e-8f;
    const int64_t ctr = (int64_t)V + qd;
    for (int m = 0; m < 3; m++) {
        const float v0 = verts[3 * q[0] + m], v1 = verts[3 * q[1] + m], v2 = verts[3 * q[2] + m], v3 = verts[3 * q[3] + m];
        verts[3 * ctr + m] = (g02 * ((v0 + v2) / 2.0f) + g13 * ((v1 + v3) / 2.0f)) / den;
    }
    for (int m = 0; m < 4; m++) {
        out[3 * m + 0] = q[m];
        out[3 * m + 1] = q[(m + 1) & 3];
        out[3 * m + 2] = ctr;
    }
}

struct BwdArgs {
    const float *x, *s, *alpha, *beta, *gamma, *verts, *gverts, *gldev;
    float *galpha, *gbeta, *ggamma;
    float4* rec;  // 24 per surface cube: (edge, end) -> (dL/ds, dL/dx) of that end through that edge; NULL: not wanted
    int res, training, n_verts, n_all, cap;
};

__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.0f : (v < 0.f ? -1.0f : 0.0f); }

__global__ __launch_bounds__(TPB) void k_wf_bwd_cube(BwdArgs A, const uint16_t* __restrict__ info, const int32_t* __restrict__ rank,
                                                     const int32_t* __restrict__ total, const int32_t* __restrict__ cid,
                                                     const int32_t* __restrict__ voff, const int32_t* __restrict__ qoff) {
    FLEXI_EDGE_TABLES
    FLEXI_RING_TABLE
    const int64_t t = gid();
    const int n = usable_count(total[0], A.cap), res = A.res;
    if (t >= n || total[1] != A.n_verts) return;
    const int64_t cube = cid[t];
    if (cube < 0 || cube >= (int64_t)res * res * res) return;
    const unsigned code = info[cube] & 255u;
    const int np = c_flexi_npatch[code], base = voff[t];
    if (base < 0 || base + np > A.n_verts) return;
    FLEXI_IJK(cube, res)
    float sc[8], xc[24], al[8], be[12];
    load_cube(A.x, A.s, A.alpha, A.beta, res, cube, sc, xc, al, be);
    float ga[8], gb[12], ggam = 0.f;
#pragma unroll
    for (int c = 0; c < 8; c++) ga[c] = 0.f;
#pragma unroll
    for (int e = 0; e < 12; e++) gb[e] = 0.f;
    const float gam_own = A.gamma ? A.gamma[cube] : 1.0f;

    for (int p = 0; p < np; p++) {
        float gv[3];
        for (int q = 0; q < 3; q++) gv[q] = A.gverts[3 * (size_t)(base + p) + q];
        const float gl = A.gldev ? A.gldev[base + p] : 0.f;
        if (A.training) {
            // the centres of the quads this dual vertex is a corner of: d centre / d v = (its diagonal's product / 2) / den, and
            // d centre / d (that product) = ((v + v_opposite) / 2 - centre) / den
#pragma unroll
            for (int e = 0; e < 12; e++) {
                if (c_flexi_edge_patch[code][e] != p) continue;
                const int axis = e / 4, r = fx_er[e];
                const int oi = i - c_flexi_ring[axis][r][0], oj = j - c_flexi_ring[axis][r][1], ok = k - c_flexi_ring[axis][r][2];
                if (oi >= res || oj >= res || ok >= res) continue;  // (never below 0: the ring's offsets are 0 or -1)
                const int64_t owner = ((int64_t)oi * res + oj) * res + ok;
                if (!((info[owner] >> (8 + axis)) & 1u)) continue;
                const int ork = rank[owner];
                if ((unsigned)ork >= (unsigned)n) continue;
                const int qd = qoff[3 * (size_t)ork + axis];
                if (qd < 0 || (int64_t)A.n_verts + qd >= A.n_all) continue;
                int64_t cc[4];
                int rk[4];
                if (!ring_of(axis, oi, oj, ok, res, rank, n, cc, rk)) continue;
                const int opp = (r + 2) & 3;
                const float g_opp = A.gamma ? A.gamma[cc[opp]] : 1.0f;
                const float g_n1 = A.gamma ? A.gamma[cc[(r + 1) & 3]] : 1.0f, g_n3 = A.gamma ? A.gamma[cc[(r + 3) & 3]] : 1.0f;
                const float mine = gam_own * g_opp, other = g_n1 * g_n3, den = (mine + other) + 1e-8f;
                const size_t ctr = (size_t)A.n_verts + qd;
                const float w = (mine / 2.0f) / den;
                float dotg = 0.f;
                const int64_t vo = (int64_t)voff[rk[opp]] + c_flexi_edge_patch[info[cc[opp]] & 255u][c_flexi_ring[axis][opp][3]];
                for (int q = 0; q < 3; q++) {
                    const float gc = A.gverts[3 * ctr + q];
                    gv[q] += gc * w;
                    if (A.ggamma && (uint64_t)vo < (uint64_t)A.n_verts) {
                        const float mid = (A.verts[3 * (size_t)(base + p) + q] + A.verts[3 * (size_t)vo + q]) / 2.0f;
                        dotg += gc * ((mid - A.verts[3 * ctr + q]) / den);
                    }
                }
                ggam += dotg * g_opp;
            }
        }
        // the forward's v, weight sum, edge count, distances to the unweighted crossings and their mean
        float v[3];
        FlexiDual fd;
        flexi_dual_vertex(code, p, sc, xc, al, be, v, nullptr, &fd);
        const float B = fd.B, cnt = fd.cnt, mean = fd.mean;
        const float* dd = fd.dd;
        float ssum = 0.f;
#pragma unroll
        for (int e = 0; e < 12; e++)
            if (c_flexi_edge_patch[code][e] == p) ssum += sign_of(dd[e] - mean);
        // dL/dd_e = gl (sign_e - ssum / n) / n; dL/dz_e = dL/dd_e (z_e - v) / d_e; dL/dv loses their sum
        float gvt[3] = {gv[0], gv[1], gv[2]};
        if (gl != 0.f) {
#pragma unroll
            for (int e = 0; e < 12; e++) {
                if (c_flexi_edge_patch[code][e] != p || !(dd[e] > 0.f)) continue;
                const int a = fx_ea[e], b = fx_eb[e];
                const float D = sc[b] - sc[a];
                const float gd = gl * ((sign_of(dd[e] - mean) - ssum / cnt) / cnt);
                for (int q = 0; q < 3; q++) gvt[q] -= gd * (((xc[3 * a + q] * sc[b] - xc[3 * b + q] * sc[a]) / D - v[q]) / dd[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 12; e++) {
            if (c_flexi_edge_patch[code][e] != p) continue;
            const int a = fx_ea[e], b = fx_eb[e];
            const float D = sc[b] - sc[a], za = sc[b] / D, zb = -sc[a] / D;
            const float wa = al[a] * sc[a], wb = al[b] * sc[b], Dw = wb - wa, ta = wb / Dw, tb = -wa / Dw;
            const float gd = (gl != 0.f && dd[e] > 0.f) ? gl * ((sign_of(dd[e] - mean) - ssum / cnt) / cnt) : 0.f;
            float gu[3], gz[3], dot_u = 0.f, dot_z = 0.f, dot_b = 0.f;
            for (int q = 0; q < 3; q++) {
                const float xa = xc[3 * a + q], xb = xc[3 * b + q];
                const float u = (xa * wb - xb * wa) / Dw;
                gu[q] = gvt[q] * (be[e] / B);
                gz[q] = gd != 0.f ? gd * (((xa * sc[b] - xb * sc[a]) / D - v[q]) / dd[e]) : 0.f;
                dot_u += gu[q] * (xa - xb);
                dot_z += gz[q] * (xa - xb);
                dot_b += gvt[q] * (u - v[q]);
            }
            gb[e] = dot_b / B;
            // 1 / D^2 as two divisions (k_flexi_bwd): |s / D| <= 1 on a crossing edge
            const float gwa = dot_u * (ta / Dw), gwb = dot_u * (tb / Dw);
            ga[a] += gwa * sc[a];
            ga[b] += gwb * sc[b];
            if (A.rec) {
                float4* rec = A.rec + ((size_t)t * 12 + e) * 2;
                rec[0] = make_float4(gwa * al[a] + dot_z * (za / D), gu[0] * ta + gz[0] * za, gu[1] * ta + gz[1] * za, gu[2] * ta + gz[2] * za);
                rec[1] = make_float4(gwb * al[b] + dot_z * (zb / D), gu[0] * tb + gz[0] * zb, gu[1] * tb + gz[1] * zb, gu[2] * tb + gz[2] * zb);
            }
        }
    }
    if (A.galpha) {
#pragma unroll
        for (int c = 0; c < 8; c++) A.galpha[8 * (size_t)cube + c] = ga[c];
    }
    if (A.gbeta) {
#pragma unroll
        for (int e = 0; e < 12; e++) A.gbeta[12 * (size_t)cube + e] = gb[e];
    }
    if (A.ggamma && A.training) A.ggamma[cube] = ggam;
}

// the gather of flexi_core.h (flexi_owns_point, flexi_walk_point; k_sf_bwd's): 8 threads per surface cube, one per corner; the owner of
// a grid point adds the record of every (ring cube, edge) in which one of its six edges crosses, and stores once.
__global__ __launch_bounds__(TPB) void k_wf_bwd_gather(const float4* __restrict__ rec, int res, int cap, const uint16_t* __restrict__ info,
                                                       const int32_t* __restrict__ rank, const int32_t* __restrict__ total,
                                                       const int32_t* __restrict__ cid, float* __restrict__ gs, float* __restrict__ gx) {
    const int n = usable_count(total[0], cap);
    const int64_t t = gid();
    if (t >= 8 * (int64_t)n) return;
    const int64_t cube = cid[t >> 3];
    if (cube < 0 || cube >= (int64_t)res * res * res) return;
    int pt[3];
    const auto is_surface = [&](int64_t c) {
        const unsigned oc = info[c] & 255u;
        return oc != 0u && oc != 255u;
    };
    if (!flexi_owns_point(cube, (int)(t & 7), res, pt, is_surface)) return;
    float as = 0.f, ax[3] = {0.f, 0.f, 0.f};
    bool any = false;
    flexi_walk_point(
        pt, res, [](int, int, int, int, int) { return true; },
        [&](int, int side, int64_t cc, int e) {
            if (c_flexi_edge_patch[info[cc] & 255u][e] < 0) return;  // the edge does not cross (or the cube is no surface cube)
            const int rk = rank[cc];
            if ((unsigned)rk >= (unsigned)n) return;
            const float4 v = rec[((size_t)rk * 12 + e) * 2 + (side ? 0 : 1)];
            as += v.x, ax[0] += v.y, ax[1] += v.z, ax[2] += v.w;
            any = true;
        });
    if (!any) return;
    const size_t gi = flexi_point(pt[0], pt[1], pt[2], res + 1);
    if (gs) gs[gi] = as;
    if (gx)
        for (int m = 0; m < 3; m++) gx[3 * gi + m] = ax[m];
}

bool res_ok(int32_t r) { return r >= 1 && r <= FOHO_WFLEXI_MAX_RES; }

}  // namespace

FOHO_SIDE_ENTRY_POINTS(wflexi, FOHO_WFLEXI_API, FOHO_WFLEXI_VERSION)

extern "C" {

FOHO_WFLEXI_API size_t foho_wflexi_workspace_bytes(int32_t res, int32_t verts_cap) {
    return (res_ok(res) && verts_cap >= 0) ? carve(nullptr, res, verts_cap).bytes : 0;
}

FOHO_WFLEXI_API size_t foho_wflexi_bwd_bytes(int32_t n_cubes) { return n_cubes >= 0 ? ((size_t)n_cubes * 24 * sizeof(float4) + 255) & ~(size_t)255 : 0; }

FOHO_WFLEXI_API int foho_wflexi_fwd(const float* x, const float* s, const float* alpha, const float* beta, const float* gamma,
                                    int32_t res, int32_t training, float* verts, int32_t verts_cap, int64_t* faces, int32_t faces_cap,
                                    float* l_dev, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !s || !verts || !faces || !counts || !workspace) return fail(-1, "foho_wflexi_fwd: null argument");
    if (!res_ok(res)) return fail(-1, "foho_wflexi_fwd: resolution outside 1 .. 256");
    if (verts_cap < 0 || faces_cap < 0) return fail(-1, "foho_wflexi_fwd: bad capacity");
    const Ws w = carve(workspace, res, verts_cap);
    if (workspace_bytes < w.bytes) return fail(-3, "foho_wflexi_fwd: workspace too small (query foho_wflexi_workspace_bytes)");
    const hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)verts_cap;
    hipLaunchKernelGGL(k_wf_classify, dim3((unsigned)w.blocks), dim3(TPB), 0, st, s, res, w.info, w.bcnt);
    hipLaunchKernelGGL(k_wf_blocks, dim3(1), dim3(TPB), 0, st, w.bcnt, (int)w.blocks, w.bpre, w.tot);
    hipLaunchKernelGGL(k_wf_offsets, dim3((unsigned)w.blocks), dim3(TPB), 0, st, w.info, res, w.bpre, w.tot, verts_cap, training, w.rank, w.cid,
                       w.voff, w.qoff, counts);
    hipLaunchKernelGGL(k_wf_verts, dim3(blocks_for(n)), dim3(TPB), 0, st, x, s, alpha, beta, res, w.info, w.tot, verts_cap, w.cid, w.voff, verts,
                       l_dev, counts);
    hipLaunchKernelGGL(k_wf_faces, dim3(blocks_for(3 * n)), dim3(TPB), 0, st, gamma, res, training, w.info, w.rank, w.tot, verts_cap, w.cid,
                       w.voff, w.qoff, verts, faces, faces_cap, counts);
    return launched("foho_wflexi_fwd");
}

FOHO_WFLEXI_API int foho_wflexi_bwd(const float* x, const float* s, const float* alpha, const float* beta, const float* gamma,
                                    int32_t res, int32_t training, const float* verts, int32_t n_verts, int32_t n_all, int32_t n_cubes,
                                    const float* grad_verts, const float* grad_l_dev, float* grad_s, float* grad_x, float* grad_alpha,
                                    float* grad_beta, float* grad_gamma, const void* workspace, size_t workspace_bytes,
                                    int32_t verts_cap, void* scratch, size_t scratch_bytes, void* stream) {
    if (!x || !s || !grad_verts || !workspace) return fail(-1, "foho_wflexi_bwd: null argument");
    if (!res_ok(res)) return fail(-1, "foho_wflexi_bwd: resolution outside 1 .. 256");
    if (n_verts < 0 || n_all < n_verts || n_cubes < 0 || n_cubes > n_verts || verts_cap < n_all)
        return fail(-1, "foho_wflexi_bwd: bad counts (0 <= n_cubes <= n_verts <= n_all <= verts_cap)");
    if ((grad_alpha && !alpha) || (grad_beta && !beta) || (grad_gamma && !gamma))
        return fail(-1, "foho_wflexi_bwd: a gradient is asked for a weight that is NULL");
    if (training && !verts) return fail(-1, "foho_wflexi_bwd: training mode needs the forward's vertices");
    const Ws w = carve(workspace, res, verts_cap);
    if (workspace_bytes < w.bytes) return fail(-3, "foho_wflexi_bwd: workspace too small (query foho_wflexi_workspace_bytes)");
    const bool want_rec = grad_s || grad_x;
    if (want_rec && (!scratch || scratch_bytes < foho_wflexi_bwd_bytes(n_cubes)))
        return fail(-3, "foho_wflexi_bwd: scratch too small (query foho_wflexi_bwd_bytes)");
    if (n_cubes == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    BwdArgs A;
    A.x = x, A.s = s, A.alpha = alpha, A.beta = beta, A.gamma = gamma, A.verts = verts, A.gverts = grad_verts, A.gldev = grad_l_dev;
    A.galpha = grad_alpha, A.gbeta = grad_beta, A.ggamma = training ? grad_gamma : nullptr;
    A.rec = want_rec ? (float4*)scratch : nullptr;
    A.res = res, A.training = training, A.n_verts = n_verts, A.n_all = n_all, A.cap = n_cubes;
    // the list is n_cubes long: a workspace of another field (another count) is refused by usable_count
    hipLaunchKernelGGL(k_wf_bwd_cube, dim3(blocks_for((size_t)n_cubes)), dim3(TPB), 0, st, A, w.info, w.rank, w.tot, w.cid, w.voff, w.qoff);
    if (want_rec)
        hipLaunchKernelGGL(k_wf_bwd_gather, dim3(blocks_for(8 * (size_t)n_cubes)), dim3(TPB), 0, st, (const float4*)scratch, res, n_cubes,
                           w.info, w.rank, w.tot, w.cid, grad_s, grad_x);
    return launched("foho_wflexi_bwd");
}

}  // extern "C"
