/*
 * foho_sflexi.h -- C ABI of libfoho_sflexi.so: the sparse FlexiCubes extractor (followmyhold_amd/sparse_flexi.py).  A library of
 * its own, next to libfoho_hip.so and libfoho_vol.so, whose ABIs stay as they are.
 *
 * The mesh foho_flexi_fwd (include/foho_hip.h) builds from a dense (res+1)^3 x 3 array of grid positions, built from three per-axis
 * coordinate tables instead, with work and memory outside the field proportional to the number of surface cubes (cubes whose 8
 * corners differ in sign under `s < 0`): the same vertices bit for bit, the same faces and l_dev, in the same order (vertices by
 * (cube, patch), faces by (axis, i, j, k) of their grid edge).  foho_sflexi_mark and foho_sflexi_extract are the forward;
 * foho_sflexi_bwd is the gradient of the vertices to the field, from what the forward left in the mark buffer and the cube workspace.
 *
 *   foho_sflexi_mark      the bit mask of the surface cubes, its prefix sums per 256 cubes, and the number of surface cubes
 *   foho_sflexi_extract   the mesh, from the mark buffer: ascending list of the surface cubes, case code and the three owned
 *                         grid edges per cube, one scan for the vertex and quad offsets, vertices and quads
 *   foho_sflexi_bwd       dL/ds from dL/dvertices by gather: one thread per corner of a surface cube, the owner of a grid point sums
 *                         its at most 24 terms in a fixed order and stores once
 *
 * The caller reads *n_cubes back between the two calls and sizes cube_cap, the cube workspace and the outputs from it (a surface
 * cube has at most 4 dual vertices and owns at most 3 quads = 6 triangles).
 *
 * Conventions: the field is float32 in the flattened "ij" layout of generate_dense_grid_points (x slowest), s < 0 inside, s == 0
 * outside; axes is 3 x (res+1) float32, point (i,j,k) at (axes[i], axes[res+1+j], axes[2(res+1)+k]); cube (i,j,k) has the id
 * (i*res + j)*res + k.  Every launch is asynchronous on the hipStream_t passed as `void* stream`; nothing synchronises and
 * nothing allocates.  Return 0 on success, a negative value otherwise, with a thread-local message in foho_sflexi_last_error().
 * No atomics except the OR into the overflow word: every output is bitwise repeatable.
 */
#ifndef FOHO_SFLEXI_H
#define FOHO_SFLEXI_H

#include <stddef.h>
#include <stdint.h>

#ifndef FOHO_SFLEXI_API
#define FOHO_SFLEXI_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FOHO_SFLEXI_VERSION 100
#define FOHO_SFLEXI_MAX_RES 1024
#define FOHO_SFLEXI_MAX_CUBES (1 << 26) /* 4 vertices and 3 quads per cube stay far inside int32 */
/* bits of counts[2] */
#define FOHO_SFLEXI_OVER_VERTS 1 /* as foho_flexi_fwd: a cube's vertices would pass verts_cap */
#define FOHO_SFLEXI_OVER_FACES 2 /* as foho_flexi_fwd: a quad's triangles would pass faces_cap */
#define FOHO_SFLEXI_OVER_CUBES 4 /* more surface cubes than cube_cap: nothing is extracted, counts[0] = counts[1] = 0 */

FOHO_SFLEXI_API int foho_sflexi_version(void);
FOHO_SFLEXI_API const char* foho_sflexi_last_error(void);

/* Bytes of the mark buffer for a res^3 grid, of the cube workspace for cube_cap surface cubes, and their sum: everything the
 * extraction needs outside the field and the outputs.  0 for an argument out of range (res 1 .. FOHO_SFLEXI_MAX_RES,
 * cube_cap 0 .. FOHO_SFLEXI_MAX_CUBES). */
FOHO_SFLEXI_API size_t foho_sflexi_mark_bytes(int32_t res);
FOHO_SFLEXI_API size_t foho_sflexi_cube_bytes(int32_t cube_cap);
FOHO_SFLEXI_API size_t foho_sflexi_workspace_bytes(int32_t res, int32_t cube_cap);

/* s: (res+1)^3.  marks: foho_sflexi_mark_bytes(res) bytes, written.  n_cubes: one int32 in device memory. */
FOHO_SFLEXI_API int foho_sflexi_mark(const float* s, int32_t res, void* marks, size_t marks_bytes, int32_t* n_cubes, void* stream);

/* marks: what foho_sflexi_mark wrote for the same s and res.  workspace: foho_sflexi_cube_bytes(cube_cap) bytes of scratch.
 * verts: verts_cap x 3, faces: faces_cap x 3 int64, l_dev: verts_cap or NULL.  counts: 3 int32 in device memory:
 * [0] vertices, [1] triangles, [2] overflow bits.  On overflow nothing is written past a capacity. */
FOHO_SFLEXI_API int foho_sflexi_extract(const float* axes, const float* s, int32_t res, const void* marks, size_t marks_bytes,
                                        int32_t cube_cap, float* verts, int32_t verts_cap, int64_t* faces, int32_t faces_cap,
                                        float* l_dev, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* dL/ds of the vertices foho_sflexi_extract wrote.  axes, s, res, marks, cube_cap and workspace: those of that call, the workspace as
 * it left it.  grad_verts: n_verts x 3, dL/dvertices.  grad_s: (res+1)^3, ZEROED BY THE CALLER: every grid point that ends a sign-
 * changing grid edge is written exactly once, with a plain store, and nothing else is touched.  Per cube, patch (dual vertex v, cnt
 * crossing edges) and crossing edge (a, b) of the patch, with D = s_b - s_a and g = grad_verts[v] / cnt:
 *   grad_s[a] += g . (x_a - x_b) (s_b / D) / D        grad_s[b] += g . (x_a - x_b) (-s_a / D) / D
 * (foho_flexi_bwd's terms; x from the axis tables, so only the edge's own axis is left of the dot product).  No float atomics: a
 * grid point's terms are summed in a fixed order, so grad_s is bitwise repeatable.  One launch, no host read: it can be captured in
 * a graph.  cube_cap == 0 or n_verts == 0: success, nothing launched.  There is no gradient to the axis tables. */
FOHO_SFLEXI_API int foho_sflexi_bwd(const float* axes, const float* s, int32_t res, const void* marks, size_t marks_bytes,
                                    int32_t cube_cap, const float* grad_verts, int32_t n_verts, float* grad_s, const void* workspace,
                                    size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
