// flexi_core.h -- the per-cube arithmetic of FlexiCubes with default weights (= Dual Marching Cubes), once, for the dense extractor
// (k_flexi.inc: every cube and grid edge of the grid) and the sparse one (foho_sflexi.hip: the surface cubes only).  Both call these
// functions under the same flags (-ffp-contract=off, correctly rounded division and sqrt), so their vertices, faces and l_dev are the
// same plain binary32 operations in the same order: bitwise equal by construction.
//
// Grid point (i,j,k) -> (i*G + j)*G + k, G = res + 1; cube corners in x-fastest order; cube edges 0-3 along x, 4-7 along y, 8-11
// along z (followmyhold_amd/flexi_tables.py).  What differs between the callers stays with them: where corner positions, vertex
// offsets and case codes come from, which end decides a quad's orientation, and the capacity checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_flexi_tables.inc"

// corner pair of every cube edge; constexpr and function-local so that the unrolled loops index the corner registers statically (a
// run-time index would push the 8 + 24 corner values into scratch memory)
#define FLEXI_EDGE_TABLES                                           \
    constexpr int fx_ea[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3}; \
    constexpr int fx_eb[12] = {1, 3, 5, 7, 2, 3, 6, 7, 4, 5, 6, 7};

// sign code of cube (i,j,k): bit c set when corner c is inside (s < 0)
__device__ __forceinline__ unsigned flexi_cube_code(const float* s, int res, int i, int j, int k) {
    const int G = res + 1;
    unsigned code = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const size_t gi = ((size_t)(i + (c & 1)) * G + (j + ((c >> 1) & 1))) * G + (k + (c >> 2));
        code |= (s[gi] < 0.0f ? 1u : 0u) << c;
    }
    return code;
}

// dual vertex of patch p of a cube with sign code `code`, corner values sc[8] and corner positions xc[24]: the mean of the zero
// crossings u_e = (x_a s_b - x_b s_a) / (s_b - s_a) of the patch's edges -> vert[3]; with ldev, the mean absolute deviation of the
// crossings' distances to it -> *ldev
__device__ __forceinline__ void flexi_dual_vertex(unsigned code, int p, const float* sc, const float* xc, float* vert, float* ldev) {
    FLEXI_EDGE_TABLES
    float acc[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
#pragma unroll
    for (int e = 0; e < 12; e++) {
        if (c_flexi_edge_patch[code][e] != p) continue;
        const int a = fx_ea[e], b = fx_eb[e];
        const float den = sc[b] - sc[a];
        for (int q = 0; q < 3; q++) acc[q] += (xc[3 * a + q] * sc[b] - xc[3 * b + q] * sc[a]) / den;
        cnt += 1.0f;
    }
    float v[3];
    for (int q = 0; q < 3; q++) {
        v[q] = acc[q] / cnt;
        vert[q] = v[q];
    }
    if (ldev) {
        float dsum = 0.f, dd[12];
#pragma unroll
        for (int e = 0; e < 12; e++) {
            dd[e] = 0.f;
            if (c_flexi_edge_patch[code][e] != p) continue;
            const int a = fx_ea[e], b = fx_eb[e];
            const float den = sc[b] - sc[a];
            float d2 = 0.f;
            for (int q = 0; q < 3; q++) {
                const float u = (xc[3 * a + q] * sc[b] - xc[3 * b + q] * sc[a]) / den - v[q];
                d2 += u * u;
            }
            dd[e] = sqrtf(d2);
            dsum += dd[e];
        }
        const float mean = dsum / cnt;
        float dev = 0.f;
#pragma unroll
        for (int e = 0; e < 12; e++)
            if (c_flexi_edge_patch[code][e] == p) dev += fabsf(dd[e] - mean);
        *ldev = dev / cnt;
    }
}

// the four cubes around an edge (cyclic; the quad's normal points along +axis) and the cube-local id of the edge in each
__constant__ signed char c_flexi_ring[3][4][4] = {
    {{0, -1, -1, 3}, {0, 0, -1, 2}, {0, 0, 0, 0}, {0, -1, 0, 1}},
    {{-1, 0, -1, 7}, {-1, 0, 0, 5}, {0, 0, 0, 4}, {0, 0, -1, 6}},
    {{-1, -1, 0, 11}, {0, -1, 0, 10}, {0, 0, 0, 8}, {-1, 0, 0, 9}}};

// the quad through the dual vertices q[0..3] of an edge's ring, oriented from the inside end of the edge to the outside end
// (near_inside: the edge's near end is the inside one) and split along its first diagonal -> six indices at o
__device__ __forceinline__ void flexi_quad(int64_t* q, bool near_inside, int64_t* o) {
    if (!near_inside) {
        const int64_t t0 = q[0], t1 = q[1];
        q[0] = q[3];
        q[1] = q[2];
        q[2] = t1;
        q[3] = t0;
    }
    o[0] = q[0];
    o[1] = q[1];
    o[2] = q[2];
    o[3] = q[0];
    o[4] = q[2];
    o[5] = q[3];
}
