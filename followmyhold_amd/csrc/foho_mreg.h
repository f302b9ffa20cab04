/*
 * foho_mreg.h -- C ABI of libfoho_mreg.so: the mesh regularisers (Laplacian smoothing, normal consistency, edge length) of one mesh,
 * fused, with the gradient to the vertices (followmyhold_amd/mesh_reg.py).  A library of its own next to libfoho_hip.so and the other
 * side libraries, whose ABIs stay as they are.
 *
 * The mesh: verts (V x 3 float32), faces (F x 3 int32, every index in [0, V), the three of a face distinct).  The index tables are
 * built once per connectivity by mesh_reg.MeshTopology (int32, in device memory):
 *   nbr_off (V + 1), nbr_idx (2E), nbr_edge (2E)   per vertex its neighbours over the E unique undirected edges, ascending, and the
 *                                                  edge id of every entry (edges are numbered by ascending (lower, higher) end)
 *   edge_off (E + 1), edge_fc (3F)                 per edge the ascending list of (face << 2 | corner opposite the edge)
 *   pairs (P x 4)                                  per pair of faces on one edge: v0 < v1 the edge's ends, a, b the opposite vertices;
 *                                                  an edge with k faces gives its k (k - 1) / 2 pairs
 *   vp_off (V + 1), vp_ent (4P)                    per vertex the ascending list of (pair << 2 | slot), slot = column of `pairs`
 *
 * Terms (pytorch3d's published formulas, restated; parity with pytorch3d is UNPINNED):
 *   per face, A B C the side lengths opposite corners 0 1 2, s = (A + B + C) / 2, area = sqrt(max(s (s-A) (s-B) (s-C), 1e-12)),
 *   cot_0 = (B^2 + C^2 - A^2) / (4 area), cyclically; W_ij = sum over the faces on edge ij of the cotangent opposite the edge;
 *   S_i = sum_j W_ij; a_i = sum of area over the faces at i.  The residual r_i by method:
 *     FOHO_MREG_UNIFORM   (1 / deg_i) sum_j v_j - v_i, 0 when deg_i = 0
 *     FOHO_MREG_COT       n_i sum_j W_ij v_j - v_i, n_i = 1 / S_i where S_i > 0, else S_i
 *     FOHO_MREG_COTCURV   (sum_j W_ij v_j - S_i v_i) 0.25 q_i, q_i = 1 / a_i where a_i > 0, else a_i
 *   lap  = (1 / V) sum_i |r_i|; W, S and a are constants of the gradient; the direction r / |r| is 0 at r = 0
 *   nc   = mean over the pairs of 1 + n0.n1 / (max(|n0|, 1e-8) max(|n1|, 1e-8)), n0 = (v1-v0) x (a-v0), n1 = (v1-v0) x (b-v0); 0 at P = 0
 *   edge = mean over the edges of (|v_i - v_j| - target_length)^2; the length's gradient at 0 is 0; 0 at E = 0
 *   total = w_edge edge + w_lap lap + w_nc nc
 * A term whose weight is 0 is not computed and is reported as 0.  V = 0 or F = 0: every term is 0 and the gradient is zero.
 *
 * Conventions: float32; caller-owned buffers; every launch is asynchronous on the hipStream_t passed as `void* stream`; nothing
 * synchronises, allocates or reads back.  Return 0 on success, a negative value otherwise (-1 bad argument, -2 launch failure), with a
 * thread-local message in foho_mreg_last_error().  No atomics: per-pair gradient records and per-row scaled directions are stored
 * once, a per-vertex pass sums them through the ascending lists, and the three scalar sums go through per-workgroup partials (a fixed
 * LDS tree) that one workgroup adds in index order -- terms, total and gradient are bitwise repeatable.  An entry of a table that
 * points outside its target is skipped, never followed.
 */
#ifndef FOHO_MREG_H
#define FOHO_MREG_H

#include <stddef.h>
#include <stdint.h>

#ifndef FOHO_MREG_API
#define FOHO_MREG_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FOHO_MREG_VERSION 100
#define FOHO_MREG_UNIFORM 0
#define FOHO_MREG_COT 1
#define FOHO_MREG_COTCURV 2
/* indices into `out` */
#define FOHO_MREG_LAP 0
#define FOHO_MREG_NC 1
#define FOHO_MREG_EDGE 2
#define FOHO_MREG_TOTAL 3

FOHO_MREG_API int foho_mreg_version(void);
FOHO_MREG_API const char* foho_mreg_last_error(void);

/* Bytes of the workspace: 32 B per vertex (the row records), 8 B per edge (W and the area sum), 64 B per pair (the gradient
 * records), 4 B per workgroup and term (the partial sums).  0 for a negative argument. */
FOHO_MREG_API size_t foho_mreg_workspace_bytes(int32_t V, int32_t E, int32_t P);

/* out: 4 float32 in device memory (FOHO_MREG_LAP, _NC, _EDGE, _TOTAL).  grad: V x 3, d total / d verts, every row written; NULL =
 * not wanted.  At most three launches, whichever terms are on: (1) per edge W and the area sum (the cot methods), per pair the term
 * and its four gradient records (w_nc != 0); (2) per vertex the residual, its norm, the scaled directions, and the vertex's share
 * of the edge term (w_lap != 0 or w_edge != 0); (3) per vertex the gather of the gradient, and one more workgroup that adds the
 * partial sums in order and writes `out`. */
FOHO_MREG_API int foho_mreg_run(const float* verts, const int32_t* faces, int32_t V, int32_t F, int32_t E, int32_t P,
                                const int32_t* nbr_off, const int32_t* nbr_idx, const int32_t* nbr_edge, const int32_t* edge_off,
                                const int32_t* edge_fc, const int32_t* pairs, const int32_t* vp_off, const int32_t* vp_ent,
                                int32_t method, float w_lap, float w_nc, float w_edge, float target_length, float* out, float* grad,
                                void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
