// foho_mreg.hip -- libfoho_mreg.so: Laplacian smoothing, normal consistency and edge length of one mesh, fused, with the gradient to the
// vertices (C ABI, formulas and table layout: foho_mreg.h; Python side: followmyhold_amd/mesh_reg.py).
//
// Three launches at most, no atomics (cdna_hip_programming's store pass + per-destination sum pass):
//   k_mreg_items    one thread per edge (cot methods): W_e and the area sum of the edge's faces, from its (face, corner) list;
//                   one thread per pair (normal consistency): the pair's term and its four gradient records, one float4 each at
//                   4 pair + slot, and the workgroup's partial sum of the terms.  The two roles share the grid: the first nb_e
//                   workgroups are edges, the next nb_p are pairs.
//   k_mreg_rows     one thread per vertex: the residual r_i over the ascending neighbour list, |r_i|, and the two scaled directions
//                   that the gradient needs -- P_i (what a neighbour reads, times W) and D_i (the diagonal part); the vertex's share
//                   of the edge term (its edges towards a higher index); the workgroup's partial sums.
//   k_mreg_gather   one thread per vertex: grad_k = s_lap (sum_i W_ki P_i - D_k) + s_edge sum_j 2 (len - t) (v_k - v_j) / len
//                   + s_nc sum over the vertex's (pair, slot) list of the records, each list in its stored order; one more
//                   workgroup adds the partial sums in index order (a strided pass per thread, then the LDS tree) and writes `out`.
// Every list is looped over, whatever its length.  Every index read from a table is checked against its target before it is used.
#include "foho_carve.h"
#include "foho_side.h"
#include "foho_mreg.h"

namespace {

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ float norm(V3 a) { return sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 load3(const float* p, int i) { return v3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }
__device__ __forceinline__ V3 xyz(float4 r) { return v3(r.x, r.y, r.z); }
__device__ __forceinline__ float4 rec(V3 a) { return make_float4(a.x, a.y, a.z, 0.f); }

struct MregArgs {
    const float* verts;
    const int32_t* faces;
    int V, F, E, P;
    const int32_t *nbr_off, *nbr_idx, *nbr_edge, *edge_off, *edge_fc, *pairs, *vp_off, *vp_ent;
    int method, lap, nc, edge;       // the method and which terms are on
    float target;
    float w_lap, w_nc, w_edge;
    float s_lap, s_nc, s_edge;       // w_lap / V, w_nc / P, w_edge / E: the gradient's scales
    float2* erec;                    // E: (W_e, area sum of the edge's faces)
    float4 *prec, *drec;             // V each: P_i and D_i
    float4* pair_rec;                // 4P: the pair's gradient at slot 0..3
    float *part_lap, *part_edge;     // nb_r each
    float* part_nc;                  // nb_p
    int nb_e, nb_p, nb_r, nb_v;      // workgroups: edge role, pair role, k_mreg_rows, the vertex part of k_mreg_gather
    float* out;
    float* grad;
};

// the workgroup's sum in a fixed tree; s: TPB floats.  Every thread of the workgroup calls it.
__device__ __forceinline__ float block_sum(float v, float* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = TPB / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    const float r = s[0];
    __syncthreads();
    return r;
}

// [beg, end) of list i of an offset table whose entries number n_entries, clipped to them
__device__ __forceinline__ void list_range(const int32_t* off, int i, int n_entries, int& beg, int& end) {
    beg = max(off[i], 0);
    end = min(off[i + 1], n_entries);
}

__device__ __forceinline__ bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }

__global__ __launch_bounds__(TPB) void k_mreg_items(MregArgs a) {
    __shared__ float s_sum[TPB];
    if ((int)blockIdx.x < a.nb_e) {      // ---- an edge: W_e and the area sum
        const int64_t e = gid();
        if (e >= a.E) return;
        int beg, end;
        list_range(a.edge_off, (int)e, 3 * a.F, beg, end);
        float W = 0.f, area_sum = 0.f;
        for (int t = beg; t < end; ++t) {
            const int ent = a.edge_fc[t], f = ent >> 2, c = ent & 3;
            if (!in_range(f, a.F) || c > 2) continue;
            const int i0 = a.faces[3 * (size_t)f], i1 = a.faces[3 * (size_t)f + 1], i2 = a.faces[3 * (size_t)f + 2];
            if (!in_range(i0, a.V) || !in_range(i1, a.V) || !in_range(i2, a.V)) continue;
            const V3 p0 = load3(a.verts, i0), p1 = load3(a.verts, i1), p2 = load3(a.verts, i2);
            const float A = norm(p1 - p2), B = norm(p0 - p2), C = norm(p0 - p1);
            const float s = 0.5f * (A + B + C);
            const float area = sqrtf(fmaxf(s * (s - A) * (s - B) * (s - C), 1e-12f));
            const float A2 = A * A, B2 = B * B, C2 = C * C;
            const float num = c == 0 ? (B2 + C2 - A2) : c == 1 ? (A2 + C2 - B2) : (A2 + B2 - C2);
            W += num / area * 0.25f;
            area_sum += area;
        }
        a.erec[e] = make_float2(W, area_sum);
        return;
    }
    // ---- a pair: 1 + cos(n0, n1) and its gradient to v0, v1, a, b
    const int64_t p = (int64_t)((int)blockIdx.x - a.nb_e) * TPB + threadIdx.x;
    float term = 0.f;
    if (p < a.P) {
        const int4 q = ((const int4*)a.pairs)[p];
        V3 g0v = v3(0, 0, 0), g1v = g0v, gav = g0v, gbv = g0v;
        if (in_range(q.x, a.V) && in_range(q.y, a.V) && in_range(q.z, a.V) && in_range(q.w, a.V)) {
            const V3 v0 = load3(a.verts, q.x);
            const V3 e = load3(a.verts, q.y) - v0, pa = load3(a.verts, q.z) - v0, pb = load3(a.verts, q.w) - v0;
            const V3 n0 = cross(e, pa), n1 = cross(e, pb);
            const float l0 = norm(n0), l1 = norm(n1);
            const float L0 = fmaxf(l0, 1e-8f), L1 = fmaxf(l1, 1e-8f);
            const float inv = 1.f / (L0 * L1);
            const float c = dot(n0, n1) * inv;
            term = 1.f + c;
            // d c / d n0 = n1 / (L0 L1) - c n0 / L0^2 where the norm is not clamped (a clamped norm is a constant)
            V3 d0 = n1 * inv, d1 = n0 * inv;
            if (l0 >= 1e-8f) d0 = d0 - n0 * (c / (L0 * L0));
            if (l1 >= 1e-8f) d1 = d1 - n1 * (c / (L1 * L1));
            // n0 = e x pa, n1 = e x pb
            g1v = cross(pa, d0) + cross(pb, d1);
            gav = cross(d0, e);
            gbv = cross(d1, e);
            g0v = v3(0, 0, 0) - (g1v + gav + gbv);
        }
        a.pair_rec[4 * p] = rec(g0v);
        a.pair_rec[4 * p + 1] = rec(g1v);
        a.pair_rec[4 * p + 2] = rec(gav);
        a.pair_rec[4 * p + 3] = rec(gbv);
    }
    const float sum = block_sum(term, s_sum);
    if (threadIdx.x == 0) a.part_nc[(int)blockIdx.x - a.nb_e] = sum;
}

__global__ __launch_bounds__(TPB) void k_mreg_rows(MregArgs a) {
    __shared__ float s_sum[TPB];
    const int64_t i = gid();
    float nr = 0.f, es = 0.f;
    if (i < a.V) {
        int beg, end;
        list_range(a.nbr_off, (int)i, 2 * a.E, beg, end);
        const V3 vi = load3(a.verts, (int)i);
        V3 acc = v3(0, 0, 0), accw = acc;      // sum_j W_ij (v_j - v_i), sum_j W_ij v_j
        float S = 0.f, area_sum = 0.f;
        int deg = 0;
        for (int t = beg; t < end; ++t) {
            const int j = a.nbr_idx[t];
            if (!in_range(j, a.V)) continue;
            const V3 vj = load3(a.verts, j);
            const V3 d = vj - vi;
            if (a.edge && j > i) {
                const float x = norm(d) - a.target;
                es += x * x;
            }
            if (!a.lap) continue;
            float w = 1.f;
            if (a.method != FOHO_MREG_UNIFORM) {
                const int e = a.nbr_edge[t];
                if (!in_range(e, a.E)) continue;
                const float2 r = a.erec[e];
                w = r.x;
                area_sum += r.y;
            }
            acc = acc + d * w;
            accw = accw + vj * w;
            S += w;
            ++deg;
        }
        if (a.lap) {
            V3 r = v3(0, 0, 0);
            float ps = 0.f, ds = 0.f;      // P_i = ps u_i, D_i = ds u_i
            if (a.method == FOHO_MREG_UNIFORM) {
                if (deg > 0) {
                    ps = 1.f / (float)deg;
                    ds = 1.f;
                    r = acc * ps;
                }
            } else if (a.method == FOHO_MREG_COT) {
                ds = 1.f;
                if (S > 0.f) {      // n_i sum_j W_ij v_j - v_i with n_i = 1 / S_i is n_i sum_j W_ij (v_j - v_i): no cancellation against v_i
                    ps = 1.f / S;
                    r = acc * ps;
                } else {
                    ps = S;
                    r = accw * ps - vi;
                }
            } else {
                const float ai = 0.5f * area_sum;      // a face at i holds two of i's edges
                ps = 0.25f * (ai > 0.f ? 1.f / ai : ai);
                ds = S * ps;
                r = acc * ps;
            }
            nr = norm(r);
            const V3 u = nr > 0.f ? r * (1.f / nr) : v3(0, 0, 0);
            a.prec[i] = rec(u * ps);
            a.drec[i] = rec(u * ds);
        }
    }
    const float sl = block_sum(nr, s_sum);
    const float se = block_sum(es, s_sum);
    if (threadIdx.x == 0) {
        a.part_lap[blockIdx.x] = sl;
        a.part_edge[blockIdx.x] = se;
    }
}

// the n partial sums in a fixed order: thread t adds t, t + TPB, ... ascending, then the tree
__device__ __forceinline__ float ordered_sum(const float* part, int n, float* s) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += TPB) acc += part[i];
    return block_sum(acc, s);
}

__global__ __launch_bounds__(TPB) void k_mreg_gather(MregArgs a) {
    __shared__ float s_sum[TPB];
    if ((int)blockIdx.x >= a.nb_v) {      // ---- the last workgroup: the terms and the total
        const float lap = a.lap ? ordered_sum(a.part_lap, a.nb_r, s_sum) / (float)a.V : 0.f;
        const float nc = a.nc ? ordered_sum(a.part_nc, a.nb_p, s_sum) / (float)a.P : 0.f;
        const float edge = a.edge ? ordered_sum(a.part_edge, a.nb_r, s_sum) / (float)a.E : 0.f;
        if (threadIdx.x == 0) {
            a.out[FOHO_MREG_LAP] = lap;
            a.out[FOHO_MREG_NC] = nc;
            a.out[FOHO_MREG_EDGE] = edge;
            a.out[FOHO_MREG_TOTAL] = a.w_edge * edge + a.w_lap * lap + a.w_nc * nc;
        }
        return;
    }
    const int64_t k = gid();
    if (k >= a.V) return;
    V3 g = v3(0, 0, 0);
    if (a.lap || a.edge) {
        int beg, end;
        list_range(a.nbr_off, (int)k, 2 * a.E, beg, end);
        const V3 vk = load3(a.verts, (int)k);
        V3 gl = v3(0, 0, 0), ge = gl;
        for (int t = beg; t < end; ++t) {
            const int j = a.nbr_idx[t];
            if (!in_range(j, a.V)) continue;
            if (a.edge) {
                const V3 d = vk - load3(a.verts, j);
                const float len = norm(d);
                if (len > 0.f) ge = ge + d * (2.f * (len - a.target) / len);
            }
            if (!a.lap) continue;
            float w = 1.f;
            if (a.method != FOHO_MREG_UNIFORM) {
                const int e = a.nbr_edge[t];
                if (!in_range(e, a.E)) continue;
                w = a.erec[e].x;
            }
            gl = gl + xyz(a.prec[j]) * w;
        }
        if (a.lap) g = (gl - xyz(a.drec[k])) * a.s_lap;
        if (a.edge) g = g + ge * a.s_edge;
    }
    if (a.nc) {
        int beg, end;
        list_range(a.vp_off, (int)k, 4 * a.P, beg, end);
        V3 gn = v3(0, 0, 0);
        for (int t = beg; t < end; ++t) {
            const int ent = a.vp_ent[t];
            if (!in_range(ent, 4 * a.P)) continue;
            gn = gn + xyz(a.pair_rec[ent]);
        }
        g = g + gn * a.s_nc;
    }
    a.grad[3 * k] = g.x;
    a.grad[3 * k + 1] = g.y;
    a.grad[3 * k + 2] = g.z;
}

constexpr int MAX_SHIFTED = (1 << 29) - 1;      // faces and pairs are stored << 2 in an int32

struct Layout {
    size_t erec, prec, drec, pair_rec, part_lap, part_edge, part_nc, total;
};

Layout layout(int V, int E, int P) {
    Carve c;
    Layout l;
    l.erec = c.take((size_t)E * sizeof(float2));
    l.prec = c.take((size_t)V * sizeof(float4));
    l.drec = c.take((size_t)V * sizeof(float4));
    l.pair_rec = c.take((size_t)P * 4 * sizeof(float4));
    l.part_lap = c.take(blocks_for((size_t)V) * sizeof(float));
    l.part_edge = c.take(blocks_for((size_t)V) * sizeof(float));
    l.part_nc = c.take(blocks_for((size_t)P) * sizeof(float));
    l.total = c.off;
    return l;
}

}  // namespace

FOHO_SIDE_ENTRY_POINTS(mreg, FOHO_MREG_API, FOHO_MREG_VERSION)

extern "C" FOHO_MREG_API size_t foho_mreg_workspace_bytes(int32_t V, int32_t E, int32_t P) {
    if (V < 0 || E < 0 || P < 0) return 0;
    return layout(V, E, P).total;
}

extern "C" FOHO_MREG_API int foho_mreg_run(const float* verts, const int32_t* faces, int32_t V, int32_t F, int32_t E, int32_t P,
                                           const int32_t* nbr_off, const int32_t* nbr_idx, const int32_t* nbr_edge,
                                           const int32_t* edge_off, const int32_t* edge_fc, const int32_t* pairs, const int32_t* vp_off,
                                           const int32_t* vp_ent, int32_t method, float w_lap, float w_nc, float w_edge,
                                           float target_length, float* out, float* grad, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    if (V < 0 || F < 0 || E < 0 || P < 0) return fail(-1, "foho_mreg_run: negative size");
    if (F > MAX_SHIFTED || P > MAX_SHIFTED || E > 2 * MAX_SHIFTED)
        return fail(-1, "foho_mreg_run: more than 2^29 - 1 faces or pairs, or 2^30 - 2 edges");
    if (method != FOHO_MREG_UNIFORM && method != FOHO_MREG_COT && method != FOHO_MREG_COTCURV)
        return fail(-1, "foho_mreg_run: unknown method " + std::to_string(method) + " (0 uniform, 1 cot, 2 cotcurv)");
    if (!out) return fail(-1, "foho_mreg_run: null out");
    const bool empty = V == 0 || F == 0;
    if (!empty && (!verts || !faces || !nbr_off || !nbr_idx || !nbr_edge || !edge_off || !edge_fc))
        return fail(-1, "foho_mreg_run: null verts, faces or neighbour / edge table");
    if (!empty && !vp_off) return fail(-1, "foho_mreg_run: null vp_off");
    if (!empty && P > 0 && (!pairs || !vp_ent)) return fail(-1, "foho_mreg_run: null pair table");
    if (!empty && E == 0) return fail(-1, "foho_mreg_run: faces without edges");
    const Layout l = layout(V, E, P);
    if (!workspace) return fail(-1, "foho_mreg_run: null workspace");
    if (workspace_bytes < l.total)
        return fail(-1, "foho_mreg_run: workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(l.total) + " needed");

    char* ws = (char*)workspace;
    MregArgs a;
    a.verts = verts, a.faces = faces, a.V = V, a.F = F, a.E = E, a.P = P;
    a.nbr_off = nbr_off, a.nbr_idx = nbr_idx, a.nbr_edge = nbr_edge, a.edge_off = edge_off, a.edge_fc = edge_fc;
    a.pairs = pairs, a.vp_off = vp_off, a.vp_ent = vp_ent;
    a.method = method;
    a.lap = !empty && w_lap != 0.f;
    a.nc = !empty && P > 0 && w_nc != 0.f;
    a.edge = !empty && w_edge != 0.f;
    a.target = target_length;
    a.w_lap = w_lap, a.w_nc = w_nc, a.w_edge = w_edge;
    a.s_lap = a.lap ? (float)((double)w_lap / V) : 0.f;
    a.s_nc = a.nc ? (float)((double)w_nc / P) : 0.f;
    a.s_edge = a.edge ? (float)((double)w_edge / E) : 0.f;
    a.erec = (float2*)(ws + l.erec), a.prec = (float4*)(ws + l.prec), a.drec = (float4*)(ws + l.drec);
    a.pair_rec = (float4*)(ws + l.pair_rec);
    a.part_lap = (float*)(ws + l.part_lap), a.part_edge = (float*)(ws + l.part_edge), a.part_nc = (float*)(ws + l.part_nc);
    a.nb_e = (a.lap && method != FOHO_MREG_UNIFORM) ? (int)blocks_for((size_t)E) : 0;
    a.nb_p = a.nc ? (int)blocks_for((size_t)P) : 0;
    a.nb_r = (a.lap || a.edge) ? (int)blocks_for((size_t)V) : 0;
    a.nb_v = (grad && V > 0) ? (int)blocks_for((size_t)V) : 0;
    a.out = out, a.grad = grad;

    hipStream_t st = (hipStream_t)stream;
    if (a.nb_e + a.nb_p > 0) hipLaunchKernelGGL(k_mreg_items, dim3((unsigned)(a.nb_e + a.nb_p)), dim3(TPB), 0, st, a);
    if (a.nb_r > 0) hipLaunchKernelGGL(k_mreg_rows, dim3((unsigned)a.nb_r), dim3(TPB), 0, st, a);
    hipLaunchKernelGGL(k_mreg_gather, dim3((unsigned)(a.nb_v + 1)), dim3(TPB), 0, st, a);
    return launched("foho_mreg_run");
}
