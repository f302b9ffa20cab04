/*
 * foho_wflexi.h -- C ABI of libfoho_wflexi.so: FlexiCubes with its three weight sets and the training-mode triangulation, forward and
 * gradient (followmyhold_amd/weighted_flexi.py).  A library of its own next to libfoho_hip.so, libfoho_vol.so, libfoho_sflexi.so and
 * libfoho_rastk.so, whose ABIs stay as they are.  foho_flexi_fwd (include/foho_hip.h) is this operator with every weight at 1.
 *
 * Orderings (this repository's, shared with oracle/flexi_ref.py and flexi_core.h): grid point (i,j,k) -> (i*G + j)*G + k, G = res + 1;
 * cube (i,j,k) -> (i*res + j)*res + k; cube corners x-fastest, corner c at (i + (c&1), j + ((c>>1)&1), k + (c>>2)); cube edges as
 * corner pairs (0,1) (2,3) (4,5) (6,7) along x, (0,2) (1,3) (4,6) (5,7) along y, (0,4) (1,5) (2,6) (3,7) along z; sign code bit c set
 * when s < 0 at corner c; patches from the table of flexi_tables.py; vertices by (cube, patch); faces by (axis, i, j, k) of their
 * grid edge; a quad only where all four cubes around the edge exist.
 *
 * Weights, already normalised and strictly positive: alpha (res^3, 8) per cube corner, beta (res^3, 12) per cube edge, gamma (res^3);
 * a NULL pointer means all ones.  For cube c and patch P (its n crossing edges e = (a, b), ascending):
 *   z_e = (x_a s_b - x_b s_a) / (s_b - s_a)                      the unweighted crossing
 *   w_a = alpha_c[a] s_a, w_b = alpha_c[b] s_b
 *   u_e = (x_a w_b - x_b w_a) / (w_b - w_a)                      the weighted crossing
 *   B = sum_e beta_c[e],  v = (sum_e beta_c[e] u_e) / B          the dual vertex
 *   d_e = |z_e - v|,  m = (sum_e d_e) / n,  l_dev = (sum_e |d_e - m|) / n
 * The deviations are taken to the UNWEIGHTED crossings: that is how kaolin 0.17.0's _compute_vd is recalled (it hands
 * zero_crossing_group to _compute_reg_loss).  Parity with kaolin is UNPINNED, here as for the rest of the operator.  kaolin returns
 * the deviations per (vertex, edge) entry; l_dev is their mean per dual vertex, as foho_flexi_fwd returns it.  With every weight 1
 * these are the operations of flexi_dual_vertex (flexi_core.h) in its order, and the library is compiled with its flags: vertices and
 * l_dev are bitwise foho_flexi_fwd's.
 *
 * Quads: oriented as flexi_quad does (reversed when the edge's near end is outside).  On the ORIENTED quad q0..q3, from the cubes
 * c0..c3: g02 = gamma_c0 gamma_c2, g13 = gamma_c1 gamma_c3.
 *   training == 0   (q0,q1,q2) (q0,q2,q3), unless g13 > g02 strictly: then (q0,q1,q3) (q3,q1,q2) -- the diagonal with the larger
 *                   product is split, as in kaolin; on an exact tie the first diagonal stays (kaolin takes the other), which keeps
 *                   foho_flexi_fwd's mesh at equal gamma.  Two triangles a quad, V vertices, no gradient to gamma.
 *   training != 0   one centre vertex per quad at index V + quad index,
 *                   centre = (g02 (v0 + v2) / 2 + g13 (v1 + v3) / 2) / ((g02 + g13) + 1e-8),
 *                   and four triangles (q0,q1,c) (q1,q2,c) (q2,q3,c) (q3,q0,c).  l_dev keeps length V.
 *
 * Conventions: float32 everywhere, s < 0 inside, s == 0 outside.  Caller-owned buffers; every launch is asynchronous on the
 * hipStream_t passed as `void* stream`; nothing synchronises, nothing allocates.  Return 0 on success, a negative value otherwise
 * (-1 bad argument, -2 launch failure, -3 buffer too small), with a thread-local message in foho_wflexi_last_error().  No atomics
 * except the OR into the overflow word: every output, the gradients included, is bitwise repeatable.
 */
#ifndef FOHO_WFLEXI_H
#define FOHO_WFLEXI_H

#include <stddef.h>
#include <stdint.h>

#ifndef FOHO_WFLEXI_API
#define FOHO_WFLEXI_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FOHO_WFLEXI_VERSION 100
#define FOHO_WFLEXI_MAX_RES 256 /* the weights are dense: this is the guidance-scale operator */
/* bits of counts[3] */
#define FOHO_WFLEXI_OVER_VERTS 1 /* the vertices (dual vertices, and centres in training mode) would pass verts_cap */
#define FOHO_WFLEXI_OVER_FACES 2 /* the triangles would pass faces_cap */

FOHO_WFLEXI_API int foho_wflexi_version(void);
FOHO_WFLEXI_API const char* foho_wflexi_last_error(void);

/* Bytes of the forward's workspace (6 B per cube, 20 B per vertex of capacity) and of the backward's scratch (384 B per surface
 * cube).  0 for an argument out of range (res 1 .. FOHO_WFLEXI_MAX_RES, capacities and counts >= 0). */
FOHO_WFLEXI_API size_t foho_wflexi_workspace_bytes(int32_t res, int32_t verts_cap);
FOHO_WFLEXI_API size_t foho_wflexi_bwd_bytes(int32_t n_cubes);

/* x: (res+1)^3 x 3, s: (res+1)^3, alpha / beta / gamma as above or NULL.  verts: verts_cap x 3, faces: faces_cap x 3 int64,
 * l_dev: verts_cap or NULL.  counts: 5 int32 in device memory: [0] dual vertices V, [1] all vertices (V, or V + quads in training
 * mode), [2] triangles, [3] overflow bits, [4] surface cubes.  The counts are the full ones whatever the capacities; on overflow
 * nothing is written past a capacity, and the caller calls again with capacities of at least counts[1] and counts[2] (the protocol
 * of foho_flexi_fwd).  Five launches: classify, scan of the 256-cube blocks, offsets and the list of surface cubes, dual vertices,
 * then centres and faces. */
FOHO_WFLEXI_API int foho_wflexi_fwd(const float* x, const float* s, const float* alpha, const float* beta, const float* gamma,
                                    int32_t res, int32_t training, float* verts, int32_t verts_cap, int64_t* faces, int32_t faces_cap,
                                    float* l_dev, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* Gradients of what foho_wflexi_fwd wrote.  x .. training, verts_cap and workspace: those of that call, the workspace as it left it;
 * verts: its vertices (n_all x 3; read in training mode only), n_verts = counts[0], n_all = counts[1], n_cubes = counts[4].
 * grad_verts: n_all x 3 (centre rows included); grad_l_dev: n_verts or NULL (zero).  Every gradient pointer may be NULL (not wanted)
 * and is otherwise ZEROED BY THE CALLER: grad_s (res+1)^3 and grad_x (res+1)^3 x 3 get one plain store per grid point that ends a
 * crossing edge of a surface cube, grad_alpha (res^3, 8) and grad_beta (res^3, 12) one row per surface cube, grad_gamma (res^3, used
 * in training mode only) one entry per surface cube.  grad_alpha / grad_beta / grad_gamma need the weight they belong to (not NULL).
 * |.| at 0 and the norm at 0 contribute 0; 1 / D^2 is two divisions, as in foho_flexi_bwd.
 * Two launches, no float atomics: the thread of a surface cube forms the cube's alpha and beta rows, gathers gamma (and, for its dual
 * vertices, the centres' gradient) over the quads of its twelve edges in ascending (patch, edge) order, and leaves one record per
 * (edge, end) in `scratch` (foho_wflexi_bwd_bytes(n_cubes) bytes); then the owner of a grid point -- the surface cube of the lowest
 * id that touches it -- sums the point's at most 24 records in the order (axis, towards -, towards +, ring position) and stores once.
 * n_cubes == 0: success, nothing launched. */
FOHO_WFLEXI_API int foho_wflexi_bwd(const float* x, const float* s, const float* alpha, const float* beta, const float* gamma,
                                    int32_t res, int32_t training, const float* verts, int32_t n_verts, int32_t n_all, int32_t n_cubes,
                                    const float* grad_verts, const float* grad_l_dev, float* grad_s, float* grad_x, float* grad_alpha,
                                    float* grad_beta, float* grad_gamma, const void* workspace, size_t workspace_bytes,
                                    int32_t verts_cap, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
