// flexi_core.h -- the per-cube arithmetic of FlexiCubes, once, for the dense extractor (k_flexi.inc: every cube and grid edge of the
// grid), the sparse one (foho_sflexi.hip: the surface cubes only) and the weighted one (foho_wflexi.hip: alpha, beta, gamma and the
// training-mode triangulation).  All call these functions under the same flags (-ffp-contract=off, correctly rounded division and
// sqrt), so their vertices, faces and l_dev are the same plain binary32 operations in the same order: bitwise equal by construction,
// the weighted ones where the weights are 1 (1 * u = u, B = n).
//
// Grid point (i,j,k) -> (i*G + j)*G + k, G = res + 1; cube corners in x-fastest order; cube edges 0-3 along x, 4-7 along y, 8-11
// along z (followmyhold_amd/flexi_tables.py).  Owned here:
//   FLEXI_IJK, flexi_point, flexi_corner           cube or grid point index -> i, j, k; grid point and cube corner -> grid index
//   flexi_cube_code                                sign code of a cube
//   flexi_dual_vertex, flexi_patch_edges           dual vertex and l_dev, with optional weights; what the backward needs of them
//   FLEXI_EDGE_TABLES, c_flexi_ring, FLEXI_RING_TABLE   edge -> corner pair; the four cubes around an edge; edge -> ring position
//   flexi_orient, flexi_split, flexi_quad          a quad's orientation, its split along either diagonal
//   flexi_owns_point, flexi_walk_point             the gather backward's ownership rule and its fixed walk over a grid point's terms
// What differs between the callers stays with them: where corner positions, vertex offsets and case codes come from, which end
// decides a quad's orientation, how the list of surface cubes is built, and the capacity checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_flexi_tables.inc"

// i, j, k of the cube (n = res) or grid point (n = G) with index id, divided in id's own type (size_t or int64_t: the caller's), and
// the three declared.  Macros like FLEXI_EDGE_TABLES: every caller compiles the very expressions it would write out
#define FLEXI_I(id, n) ((int)((id) / ((decltype(id))(n) * (n))))
#define FLEXI_J(id, n) ((int)(((id) / (n)) % (n)))
#define FLEXI_K(id, n) ((int)((id) % (n)))
#define FLEXI_IJK(id, n) const int k = FLEXI_K(id, n), j = FLEXI_J(id, n), i = FLEXI_I(id, n);

// grid index of grid point (i, j, k), and of corner c of cube (i, j, k)
__device__ __forceinline__ size_t flexi_point(int i, int j, int k, int G) { return ((size_t)i * G + j) * G + k; }
__device__ __forceinline__ size_t flexi_corner(int i, int j, int k, int c, int G) {
    return flexi_point(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2), G);
}

// sign code of cube (i,j,k): bit c set when corner c is inside (s < 0)
__device__ __forceinline__ unsigned flexi_cube_code(const float* s, int res, int i, int j, int k) {
    const int G = res + 1;
    unsigned code = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) code |= (s[flexi_corner(i, j, k, c, G)] < 0.0f ? 1u : 0u) << c;
    return code;
}

// corner pair of every cube edge; constexpr and function-local so that the unrolled loops index the corner registers statically (a
// run-time index would push the 8 + 24 corner values into scratch memory)
#define FLEXI_EDGE_TABLES                                           \
    constexpr int fx_ea[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3}; \
    constexpr int fx_eb[12] = {1, 3, 5, 7, 2, 3, 6, 7, 4, 5, 6, 7};

// the four cubes around an edge (cyclic; the quad's normal points along +axis) and the cube-local id of the edge in each
__constant__ signed char c_flexi_ring[3][4][4] = {
    {{0, -1, -1, 3}, {0, 0, -1, 2}, {0, 0, 0, 0}, {0, -1, 0, 1}},
    {{-1, 0, -1, 7}, {-1, 0, 0, 5}, {0, 0, 0, 4}, {0, 0, -1, 6}},
    {{-1, -1, 0, 11}, {0, -1, 0, 10}, {0, 0, 0, 8}, {-1, 0, 0, 9}}};
// ... read the other way: cube edge e runs along axis e / 4 and is the edge of ring position fx_er[e] there, the r with
// c_flexi_ring[e / 4][r][3] == e; so the cube that owns the edge's quad sits at minus that ring offset
#define FLEXI_RING_TABLE constexpr int fx_er[12] = {2, 3, 1, 0, 2, 1, 3, 0, 2, 3, 1, 0};

// number of edges in patch p of a cube with sign code `code`
__device__ __forceinline__ float flexi_patch_edges(unsigned code, int p) {
    float cnt = 0.f;
#pragma unroll
    for (int e = 0; e < 12; e++) cnt += (c_flexi_edge_patch[code][e] == p) ? 1.0f : 0.0f;
    return cnt;
}

// what a backward needs of a dual vertex: the weight sum, the edge count, the distances to the unweighted crossings and their mean
struct FlexiDual {
    float B, cnt, dd[12], mean;
};

// dual vertex of patch p of a cube with sign code `code`, corner values sc[8] and corner positions xc[24], corner weights al[8] and
// edge weights be[12]: v = (sum beta_e u_e) / sum beta_e over the patch's weighted zero crossings
// u_e = (x_a w_b - x_b w_a) / (w_b - w_a), w = alpha s -> vert[3]; with ldev or keep, the mean absolute deviation of the distances from
// v to the UNWEIGHTED crossings -> *ldev, and what led to it -> *keep
__device__ __forceinline__ void flexi_dual_vertex(unsigned code, int p, const float* sc, const float* xc, const float* al, const float* be,
                                                  float* vert, float* ldev, FlexiDual* keep = nullptr) {
    FLEXI_EDGE_TABLES
    float acc[3] = {0.f, 0.f, 0.f}, B = 0.f, cnt = 0.f;
#pragma unroll
    for (int e = 0; e < 12; e++) {
        if (c_flexi_edge_patch[code][e] != p) continue;
        const int a = fx_ea[e], b = fx_eb[e];
        const float wa = al[a] * sc[a], wb = al[b] * sc[b];
        const float den = wb - wa;
        for (int q = 0; q < 3; q++) acc[q] += be[e] * ((xc[3 * a + q] * wb - xc[3 * b + q] * wa) / den);
        B += be[e];
        cnt += 1.0f;
    }
    float v[3];
    for (int q = 0; q < 3; q++) {
        v[q] = acc[q] / B;
        vert[q] = v[q];
    }
    if (!ldev && !keep) return;
    FlexiDual d;
    d.B = B, d.cnt = cnt;
    float dsum = 0.f;
#pragma unroll
    for (int e = 0; e < 12; e++) {
        d.dd[e] = 0.f;
        if (c_flexi_edge_patch[code][e] != p) continue;
        const int a = fx_ea[e], b = fx_eb[e];
        const float den = sc[b] - sc[a];
        float d2 = 0.f;
        for (int q = 0; q < 3; q++) {
            const float u = (xc[3 * a + q] * sc[b] - xc[3 * b + q] * sc[a]) / den - v[q];
            d2 += u * u;
        }
        d.dd[e] = sqrtf(d2);
        dsum += d.dd[e];
    }
    d.mean = dsum / cnt;
    if (ldev) {
        float dev = 0.f;
#pragma unroll
        for (int e = 0; e < 12; e++)
            if (c_flexi_edge_patch[code][e] == p) dev += fabsf(d.dd[e] - d.mean);
        *ldev = dev / cnt;
    }
    if (keep) *keep = d;
}

// ... with default weights: the mean of the crossings.  The unit weights are compile-time constants, 1 * u folds to u and the weight
// sum to the edge count, so this compiles to the plain mean's instructions
__device__ __forceinline__ void flexi_dual_vertex(unsigned code, int p, const float* sc, const float* xc, float* vert, float* ldev) {
    constexpr float one[12] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    flexi_dual_vertex(code, p, sc, xc, one, one, vert, ldev);
}

// the quad through the dual vertices of an edge's ring runs from the inside end of the edge to the outside end: reverse the four
// per-cube items q[0..3] (vertex ids, gammas) when the edge's near end is not the inside one
template <typename T>
__device__ __forceinline__ void flexi_orient(T* q, bool near_inside) {
    if (!near_inside) {
        const T t0 = q[0], t1 = q[1];
        q[0] = q[3];
        q[1] = q[2];
        q[2] = t1;
        q[3] = t0;
    }
}

// the two triangles of the oriented quad q[0..3], split along its first diagonal (0-2) or its second (1-3) -> six indices at o
__device__ __forceinline__ void flexi_split(const int64_t* q, bool second, int64_t* o) {
    o[0] = q[0];
    o[1] = q[1];
    o[2] = second ? q[3] : q[2];
    o[3] = second ? q[3] : q[0];
    o[4] = second ? q[1] : q[2];
    o[5] = second ? q[2] : q[3];
}

// with default weights: oriented, first diagonal
__device__ __forceinline__ void flexi_quad(int64_t* q, bool near_inside, int64_t* o) {
    flexi_orient(q, near_inside);
    flexi_split(q, false, o);
}

// ---- the gather backward: every grid point P that ends a crossing edge is a corner of a surface cube, and the surface cube of the
// lowest id that touches P owns it.  pt[3] <- the grid point of corner q of `cube`; true when no in-grid cube around it with a lower
// id is a surface cube (is_surface(cube id), the caller's)
template <typename F>
__device__ __forceinline__ bool flexi_owns_point(int64_t cube, int q, int res, int* pt, F is_surface) {
    FLEXI_IJK(cube, res)
    pt[0] = i + (q & 1), pt[1] = j + ((q >> 1) & 1), pt[2] = k + (q >> 2);
#pragma unroll
    for (int o = 0; o < 8; o++) {
        const int ci = pt[0] - (o & 1), cj = pt[1] - ((o >> 1) & 1), ck = pt[2] - (o >> 2);
        if (ci < 0 || cj < 0 || ck < 0 || ci >= res || cj >= res || ck >= res) continue;
        const int64_t other = ((int64_t)ci * res + cj) * res + ck;
        if (other < cube && is_surface(other)) return false;
    }
    return true;
}

// the owner's walk, whose order is what makes the sum repeatable: P's six grid edges, axis 0 towards -, +, then axis 1, axis 2, and
// per edge the in-grid cubes of its ring in c_flexi_ring order.  The edge runs from grid point (mi,mj,mk) (its lower end, corner a)
// along +axis; P is a when side == 1.  edge(axis, side, mi, mj, mk) says whether to walk its ring; ring(axis, side, cube id, the
// edge's cube-local id) adds the caller's term
template <typename FE, typename FR>
__device__ __forceinline__ void flexi_walk_point(const int* pt, int res, FE edge, FR ring) {
#pragma unroll
    for (int axis = 0; axis < 3; axis++) {
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const int m = pt[axis] - 1 + side;
            if (m < 0 || m >= res) continue;
            const int mi = axis == 0 ? m : pt[0], mj = axis == 1 ? m : pt[1], mk = axis == 2 ? m : pt[2];
            if (!edge(axis, side, mi, mj, mk)) continue;
            for (int r = 0; r < 4; r++) {
                const int ci = mi + c_flexi_ring[axis][r][0], cj = mj + c_flexi_ring[axis][r][1], ck = mk + c_flexi_ring[axis][r][2];
                if (ci < 0 || cj < 0 || ck < 0 || ci >= res || cj >= res || ck >= res) continue;  // boundary edge: fewer than four cubes
                ring(axis, side, ((int64_t)ci * res + cj) * res + ck, (int)c_flexi_ring[axis][r][3]);
            }
        }
    }
}
