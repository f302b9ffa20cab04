/*
 * foho_vol.h -- C ABI of libfoho_vol.so: the index and field kernels of the hierarchical final decode
 * (followmyhold_amd/volume.py).  A library of its own, next to libfoho_hip.so, whose ABI stays as it is.
 *
 * The decoder runs between these calls (volume.py): a level selects the grid points to decode, the caller decodes them and
 * scatters the logits into the field the level filled from the coarser one.
 *
 *   foho_vol_mark     cells of a coarse (r+1)^3 field whose 8 corners are mixed under `logit > 0`, dilated by `band` cells
 *   foho_vol_select   the (2r+1)^3 points of the next level inside an active coarse cell and not already decoded there
 *   foho_vol_close    the final level's closure: undecoded corners of the 27 cubes around every sign-changing cube that has an
 *                     undecoded corner (or, with FOHO_VOL_CLOSE_ALL, every undecoded point)
 *   foho_vol_count    per-workgroup counts of a point mask, their exclusive scan and the total (device memory)
 *   foho_vol_emit     ascending int32 indices and fp16-rounded xyz of a point mask (positions of foho_vol_count)
 *   foho_vol_fill     the (2r+1)^3 field from the (r+1)^3 one: values at even indices, midpoint means of 2 / 4 / 8 corners else
 *   foho_vol_scatter  field[idx[n]] = vals[n]
 *
 * Conventions: fields are float32 in the flattened "ij" layout of generate_dense_grid_points (x slowest); a point or cell mask
 * is a uint64 array, bit p % 64 of word p / 64 for point p, ceil(n / 64) words.  Every launch is asynchronous on the
 * hipStream_t passed as `void* stream`; nothing synchronises and nothing allocates.  Return 0 on success, a negative value
 * otherwise, with a thread-local message in foho_vol_last_error().  No atomics: every output is bitwise repeatable.
 */
#ifndef FOHO_VOL_H
#define FOHO_VOL_H

#include <stddef.h>
#include <stdint.h>

#ifndef FOHO_VOL_API
#define FOHO_VOL_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FOHO_VOL_VERSION 100
#define FOHO_VOL_MAX_RES 1024          /* (1025)^3 points still fit int32 indices */
#define FOHO_VOL_CLOSE_ALL 1

FOHO_VOL_API int foho_vol_version(void);
FOHO_VOL_API const char* foho_vol_last_error(void);

/* field: (r+1)^3.  mixed, active: ceil(r^3 / 64) words each (mixed is scratch). */
FOHO_VOL_API int foho_vol_mark(const float* field, int32_t r, int32_t band, uint64_t* mixed, uint64_t* active, void* stream);

/* active: the r^3 cell mask of foho_vol_mark; coarse_decoded: (r+1)^3 point mask of the points whose value is exact.
 * sel, fine_decoded: (2r+1)^3 point masks -- the points to decode, and those plus the exact points carried over. */
FOHO_VOL_API int foho_vol_select(const uint64_t* active, const uint64_t* coarse_decoded, int32_t r, uint64_t* sel,
                                 uint64_t* fine_decoded, void* stream);

/* field: (R+1)^3; decoded: its point mask, updated in place (|= sel).  bad, near: ceil(R^3 / 64) words of scratch.
 * mode 0: closure; FOHO_VOL_CLOSE_ALL: every undecoded point (the dense fall-back). */
FOHO_VOL_API int foho_vol_close(const float* field, uint64_t* decoded, int32_t R, int32_t mode, uint64_t* bad, uint64_t* near,
                                uint64_t* sel, void* stream);

/* Workgroups foho_vol_count uses for n_points (the length of block_offsets). */
FOHO_VOL_API int64_t foho_vol_count_blocks(int64_t n_points);
/* block_offsets: foho_vol_count_blocks(n_points) int32; total: one int32. */
FOHO_VOL_API int foho_vol_count(const uint64_t* sel, int64_t n_points, int32_t* block_offsets, int32_t* total, void* stream);

/* sel over the (r+1)^3 points of a level of a grid of final resolution R (R % r == 0); tables: 3 x (R+1) float32, the
 * fp16-rounded axis coordinates of the final grid (point (i,j,k) of the level sits at x[i * R / r], y[j * R / r], z[k * R / r]).
 * idx: total int32, xyz: total x 3 float32. */
FOHO_VOL_API int foho_vol_emit(const uint64_t* sel, int32_t r, int32_t R, const float* tables, const int32_t* block_offsets,
                               int32_t* idx, float* xyz, void* stream);

/* coarse: (r+1)^3, fine: (2r+1)^3 */
FOHO_VOL_API int foho_vol_fill(const float* coarse, int32_t r, float* fine, void* stream);

FOHO_VOL_API int foho_vol_scatter(const int32_t* idx, const float* vals, int64_t n, float* field, void* stream);

#ifdef __cplusplus
}
#endif
#endif
