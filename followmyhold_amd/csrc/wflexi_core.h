// wflexi_core.h -- the per-cube arithmetic FlexiCubes adds to flexi_core.h once the weights are not all 1 (foho_wflexi.hip; semantics
// and orderings: foho_wflexi.h).  flexi_core.h stays what the other libraries compile; with unit weights the functions here perform
// its operations in its order (1 * u = u, B = n), so under the same flags their results are bitwise flexi_dual_vertex's and flexi_quad's.
#pragma once
#include "flexi_core.h"

// cube edge e runs along axis e / 4 and is the edge of ring position fx_er[e] of c_flexi_ring[e / 4]
#define WFLEXI_RING_TABLE constexpr int fx_er[12] = {2, 3, 1, 0, 2, 1, 3, 0, 2, 3, 1, 0};

// dual vertex of patch p with corner weights al[8] and edge weights be[12]: v = (sum beta_e u_e) / sum beta_e over the weighted
// crossings u_e -> vert[3], the weight sum -> *Bsum; with ldev, the mean absolute deviation of the distances from v to the UNWEIGHTED
// crossings z_e -> *ldev
__device__ __forceinline__ void wflexi_dual_vertex(unsigned code, int p, const float* sc, const float* xc, const float* al, const float* be,
                                                   float* vert, float* Bsum, float* ldev) {
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
    if (Bsum) *Bsum = B;
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

// the two triangles of the ORIENTED quad q[0..3] whose cubes carry g[0..3]: the first diagonal (flexi_quad's) unless the product over
// the second is strictly larger -> six indices at o
__device__ __forceinline__ void wflexi_split(const int64_t* q, const float* g, int64_t* o) {
    const bool second = g[1] * g[3] > g[0] * g[2];
    o[0] = q[0];
    o[1] = q[1];
    o[2] = second ? q[3] : q[2];
    o[3] = second ? q[3] : q[0];
    o[4] = second ? q[1] : q[2];
    o[5] = second ? q[2] : q[3];
}
