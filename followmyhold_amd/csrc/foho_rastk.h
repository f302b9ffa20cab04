/*
 * foho_rastk.h -- C ABI of libfoho_rastk.so: the K-fragment rasteriser behind the pytorch3d facade (ops.raster_k_fwd / raster_k,
 * facade.RasterizationSettings(k_fragments=True)).  A library of its own, next to libfoho_hip.so, libfoho_vol.so and
 * libfoho_sflexi.so, whose ABIs stay as they are.
 *
 * What pytorch3d's rasterize_meshes(faces_per_pixel = K) returns for one mesh, materialised: per pixel the K nearest fragments,
 * nearest first -- face id, depth, signed squared edge distance, perspective-correct clipped barycentrics -- padded with -1,
 * with the near-plane clipping (z = znear / 2 = 0.005) and the neighbour rule of MeshRasterizer.  foho_raster_fwd
 * (include/foho_hip.h) keeps one fragment per pixel in a 64-bit atomicMax plane; this one is pixel parallel over binned faces:
 *
 *   setup    one thread per face: NDC gather, near-plane cull / clip, tile box (8x8-pixel tiles) of the blur-inflated pixel box,
 *            faces per tile (integer atomics)
 *   scan     exclusive scan of the tile counts; the packed lists need hdr[0] entries
 *   fill     the per-tile face lists (integer atomics on a cursor; the order inside a list is free, see below)
 *   select   one wave per tile, one lane per pixel: the tile's faces stream through LDS in chunks of 64, every lane evaluates
 *            them in the oracle's operation order and keeps the K smallest keys (z bits << 32 | face id << 1 | sub-triangle) in
 *            an LDS slab; the lane then sorts its keys, re-evaluates the kept fragments and writes the K planes
 *
 * The key order (z, face id, sub-triangle) is total, so the selection does not depend on the order faces are visited in: the
 * forward pass is bitwise repeatable.  Two stated deviations from the naive rasteriser's running buffer:
 * fragments of exactly equal depth are ordered and cut by (face id, sub-triangle); and of the two halves of a face with one
 * vertex behind the near plane the one with the smaller |distance| is chosen BEFORE insertion (first half on a tie).
 *
 * Conventions: verts_ndc (V,3) float32 rows (x_ndc, y_ndc, z_view), faces (F,3) int32, as foho_raster_fwd; pixel (0,0) is the
 * top-left one, +X left, +Y up.  Perspective-correct and clipped barycentrics are always on.  Every launch is asynchronous on
 * the hipStream_t passed as `void* stream`; nothing synchronises and nothing allocates.  Return 0 on success, a negative value
 * otherwise, with a thread-local message in foho_rastk_last_error().  The forward pass uses integer atomics only; the backward
 * pass adds with float atomics, like foho_raster_bwd.
 */
#ifndef FOHO_RASTK_H
#define FOHO_RASTK_H

#include <stddef.h>
#include <stdint.h>

#ifndef FOHO_RASTK_API
#define FOHO_RASTK_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FOHO_RASTK_VERSION 101 /* 101 = foho_rastk_blend_fwd / _bwd */
#define FOHO_RASTK_MAX_K 128
#define FOHO_RASTK_MAX_LIST (1 << 30) /* entries of the packed tile lists */
#define FOHO_RASTK_BLEND_MAX_D 4 /* channels of the face attributes foho_rastk_blend_* takes */
/* flags of foho_rastk_fwd */
#define FOHO_RASTK_CULL_BACKFACES 1
/* flags of foho_rastk_blend_fwd / _bwd */
#define FOHO_RASTK_BLEND_UNIT_BARY 1  /* weights (1, 1, 1) in place of the barycentrics (PhongNormalShader); bary may be NULL */
#define FOHO_RASTK_BLEND_ALPHA_ONLY 2 /* the silhouette alpha alone: out is (H,W); face_attr, zbuf, bary, background may be NULL */
/* bits of *overflow */
#define FOHO_RASTK_OVER_LIST 1 /* the tile lists need more than list_cap entries: no output was written */

FOHO_RASTK_API int foho_rastk_version(void);
FOHO_RASTK_API const char* foho_rastk_last_error(void);

/* Bytes of workspace for one forward call.  list_cap: capacity of the packed per-tile face lists, in entries (one entry per
 * (face, 8x8 tile its pixel box overlaps) pair).  0 for an argument out of range: V, F >= 1, F <= 2^30, 1 <= H, W <= 8192,
 * H W <= 2^25, 1 <= K <= FOHO_RASTK_MAX_K, 0 <= list_cap <= FOHO_RASTK_MAX_LIST. */
FOHO_RASTK_API size_t foho_rastk_workspace_bytes(int32_t V, int32_t F, int32_t H, int32_t W, int32_t K, int64_t list_cap);

/* pix_to_face: int64 (H,W,K); zbuf, dists: float32 (H,W,K); bary: float32 (H,W,K,3); background entries are -1 in all four.
 * counts: int32 (H,W), the fragments the pixel received before the cut at K (NULL: not wanted).  overflow: one int32 in device
 * memory, written by every call.  When bit FOHO_RASTK_OVER_LIST is set no output was written; the first int64 of the workspace
 * then (and after every call) holds the number of list entries the scene needs: call again with that list_cap.
 * list_cap is the capacity the workspace was sized for (foho_rastk_workspace_bytes' last argument): the workspace layout depends on
 * it, so the call takes it explicitly.
 * K outside 1 .. FOHO_RASTK_MAX_K is an error (-1), not a clamp.  A face with a vertex index outside 0 .. V-1 leaves no fragment. */
FOHO_RASTK_API int foho_rastk_fwd(const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                                  float blur_radius, int32_t flags, int64_t* pix_to_face, float* zbuf, float* bary, float* dists,
                                  int32_t* counts, int32_t* overflow, int64_t list_cap, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* grad_verts_ndc (V,3) += d(zbuf, bary, dists) / d verts_ndc of every one of the H W K fragments with pix_to_face >= 0: the
 * per-fragment derivative of foho_raster_bwd (grad_bary refers to the barycentrics foho_rastk_fwd returns, the unclipped face's
 * also on a face cut by the near plane; the cut and the conversion's crossing weights move with the vertices).  grad_zbuf, grad_dists: (H,W,K), grad_bary: (H,W,K,3); any
 * of the three may be NULL.  blur_radius: the forward call's. */
FOHO_RASTK_API int foho_rastk_bwd(const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                                  const int64_t* pix_to_face, const float* grad_zbuf, const float* grad_bary, const float* grad_dists,
                                  float* grad_verts_ndc, float blur_radius, void* stream);

/* interpolate_face_attributes + softmax_rgb_blend (pytorch3d.renderer.blending) over K planes, one launch; no workspace, no
 * allocation, no host read of device memory.  Per pixel, over its fragments k:
 *   p_k = sigmoid(-dists_k / sigma)                        alpha = 1 - prod_k (1 - p_k)
 *   zinv_k = (zfar - zbuf_k) / (zfar - znear)              m = max(max_k zinv_k, 1e-10)
 *   w_k = p_k exp((zinv_k - m) / gamma)                    delta = max(exp((1e-10 - m) / gamma), 1e-10)
 *   c_k = sum_j bary_kj face_attr[pix_to_face_k, j, :]     rgb = (sum_k w_k c_k + delta background) / (sum_k w_k + delta)
 * pix_to_face: int64 (H,W,K); zbuf, dists: float32 (H,W,K); bary: (H,W,K,3); face_attr: (F,3,D) float32, 1 <= D <=
 * FOHO_RASTK_BLEND_MAX_D; background: D floats in HOST memory, read at call time; out: (H,W,D+1) float32, the D blended channels, then
 * alpha.  With FOHO_RASTK_BLEND_ALPHA_ONLY out is (H,W) alpha, F, gamma, znear, zfar are not used, and D is any legal value.
 *
 * CONTRACT ON THE PLANES: they are FRONT-PACKED, as foho_rastk_fwd writes them -- a pixel's fragments are its leading entries with
 * an id >= 0.  Everything from the first negative id on is ignored, whatever it holds (other ids, NaN), and receives no gradient;
 * planes with a valid entry behind a negative one are not pytorch3d's masked blend.  An id >= F ends the pixel's fragments like a
 * negative one (no face attribute is read out of range).  A pixel without a fragment gives rgb = background, alpha = 0.
 *
 * Refused with a negative status, never clamped: K outside 1 .. FOHO_RASTK_MAX_K, D outside 1 .. FOHO_RASTK_BLEND_MAX_D, F, H or W out
 * of foho_rastk_workspace_bytes' range, sigma <= 0, gamma <= 0, zfar <= znear, an unknown flag bit, a NULL required pointer. */
FOHO_RASTK_API int foho_rastk_blend_fwd(const int64_t* pix_to_face, const float* zbuf, const float* bary, const float* dists,
                                        const float* face_attr, int32_t F, int32_t H, int32_t W, int32_t K, int32_t D, float sigma,
                                        float gamma, float znear, float zfar, const float* background, int32_t flags, float* out,
                                        void* stream);

/* The derivative of foho_rastk_blend_fwd, the clamps and the max followed as written (the gradient through m goes to the FIRST fragment
 * of the largest zinv; where delta is clamped m does not cancel).  grad_out: (H,W,D+1), or (H,W) with FOHO_RASTK_BLEND_ALPHA_ONLY.
 * grad_zbuf, grad_dists: (H,W,K), grad_bary: (H,W,K,3), grad_face_attr: (F,3,D); any of the four may be NULL (with
 * FOHO_RASTK_BLEND_UNIT_BARY grad_bary is not written, with FOHO_RASTK_BLEND_ALPHA_ONLY only grad_dists is).  The three plane gradients
 * are WRITTEN, at the pixel's fragments only: the caller supplies zeroed buffers.  grad_face_attr is ADDED to with float atomics, like
 * foho_rastk_bwd's vertex gradient; everything else has one owner thread per entry and is bitwise repeatable. */
FOHO_RASTK_API int foho_rastk_blend_bwd(const int64_t* pix_to_face, const float* zbuf, const float* bary, const float* dists,
                                        const float* face_attr, int32_t F, int32_t H, int32_t W, int32_t K, int32_t D, float sigma,
                                        float gamma, float znear, float zfar, const float* background, int32_t flags,
                                        const float* grad_out, float* grad_zbuf, float* grad_bary, float* grad_dists,
                                        float* grad_face_attr, void* stream);

/* foho_rastk_fwd and foho_rastk_blend_fwd in one: mesh -> blended image, without the (H,W,K) planes in memory.  The bins are
 * foho_rastk_fwd's (the same workspace, foho_rastk_workspace_bytes, overflow and list_cap protocol: with FOHO_RASTK_OVER_LIST set no
 * output was written and the workspace's first int64 holds the list_cap to call again with); the wave that selected and sorted a
 * tile's K nearest keys then blends every pixel's column where it lies, in LDS.  out: (H,W,D+1) float32, or (H,W) with
 * FOHO_RASTK_BLEND_ALPHA_ONLY; BITWISE what foho_rastk_blend_fwd gives on the planes of foho_rastk_fwd for the same arguments (one
 * copy of the arithmetic, the same key order at the cut).  counts: int32 (H,W) as foho_rastk_fwd's, or NULL.  face_attr: (F,3,D), the
 * F of the mesh; background: D floats in HOST memory (both may be NULL with FOHO_RASTK_BLEND_ALPHA_ONLY).  raster_flags:
 * FOHO_RASTK_CULL_BACKFACES; blend_flags: FOHO_RASTK_BLEND_UNIT_BARY, FOHO_RASTK_BLEND_ALPHA_ONLY.  Memory: the workspace; nothing is
 * proportional to K.  Asynchronous, no allocation, no host read.  The workspace must be kept, untouched, for foho_rastk_render_bwd.
 * Refused with a negative status, never clamped: what foho_rastk_fwd and foho_rastk_blend_fwd refuse. */
FOHO_RASTK_API int foho_rastk_render_fwd(const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                                         float blur_radius, int32_t raster_flags, const float* face_attr, int32_t D, float sigma, float gamma,
                                         float znear, float zfar, const float* background, int32_t blend_flags, float* out, int32_t* counts,
                                         int32_t* overflow, int64_t list_cap, void* workspace, size_t workspace_bytes, void* stream);

/* The derivative of foho_rastk_render_fwd: grad_out (H,W,D+1), or (H,W) with FOHO_RASTK_BLEND_ALPHA_ONLY, -> grad_verts_ndc (V,3) and
 * grad_face_attr (F,3,D), both ADDED to with float atomics; either may be NULL and its work is skipped (with
 * FOHO_RASTK_BLEND_ALPHA_ONLY grad_face_attr is not touched).  Every other argument is the forward call's, and workspace is the one
 * that call left: its tile lists are read, nothing is binned again.  The per-fragment gradients are foho_rastk_blend_bwd's and go
 * straight into foho_rastk_bwd's per-fragment derivative; no plane-sized buffer exists. */
FOHO_RASTK_API int foho_rastk_render_bwd(const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                                         float blur_radius, int32_t raster_flags, const float* face_attr, int32_t D, float sigma, float gamma,
                                         float znear, float zfar, const float* background, int32_t blend_flags, const float* grad_out,
                                         float* grad_verts_ndc, float* grad_face_attr, int64_t list_cap, const void* workspace,
                                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
