// foho_rastk.hip -- libfoho_rastk.so: the K-fragment rasteriser (foho_rastk.h, ops.raster_k_fwd / raster_k_bwd).
//
// foho_raster_fwd (k_raster.inc) is face parallel with one 64-bit atomicMax per fragment: one fragment per pixel.  K fragments per
// pixel need the pixel to see all of its faces, so this one is pixel parallel over binned faces:
//   k_rk_setup    one thread per face: gather, near-plane cull / clip flag, the tile box (8x8-pixel tiles) of the blur-inflated
//                 pixel box (conservative by a pixel: the per-pixel evaluation tests the exact box again), faces per tile
//   k_rk_scan     one workgroup: exclusive scan of the tile counts -> list offsets, the cursors, the total (hdr.need); more
//                 entries than list_cap: the overflow bit, and the two kernels after it leave at once
//   k_rk_fill     one thread per face: its id into the list of every tile of its box (integer atomicAdd on the tile's cursor)
//   k_rk_select   one wave per tile, one lane per pixel; chunks of 64 faces through LDS; K smallest keys per lane in an LDS slab
//                 [slot][lane] (8-byte words, lane contiguous: conflict free), its current maximum in registers; then the lane
//                 sorts its column, re-evaluates the kept fragments from their keys and writes the planes
//   k_rk_bwd      one thread per (pixel, k): foho_raster_bwd's derivative, float atomicAdd into the vertex gradient
//   k_rk_blend_*  rastk_blend.inc: the consumer of the planes, shading and softmax blend with gradient, one thread per pixel
//   k_rk_render_* rastk_render.inc: selection and blend in one kernel each way, mesh -> image -> vertex gradient without the planes
// Compiled with foho_step.hip's flags (-ffp-contract=off, correctly rounded division and sqrt): the per-(pixel, face) arithmetic is
// foho_common.h's eval_frag / clip_subtris / subtri_bary_to_face, the functions k_raster.inc's evaluate stage and k_raster_export
// call, and that arithmetic decides face ids.
// The error plumbing and the workgroup scan are foho_side.h's; the workspace allocator is foho_carve.h's.
#include <math.h>

#include "foho_carve.h"
#include "foho_common.h"
#include "foho_rastk.h"
#include "foho_side.h"

namespace {

using namespace foho;

constexpr int TILE = 8;          // 8x8 pixels = one wave
constexpr int CH = 64;           // faces per LDS chunk of k_rk_select
constexpr float Z_CLIP = 0.01f * 0.5f;  // znear / 2 of the path's camera, as foho_raster_fwd / _bwd

struct Hdr {
    long long need;  // list entries the scene needs
    int abort;       // need > list_cap: fill and select leave at once
    int pad;
};

struct Ws {
    Hdr* hdr;
    float* face_ndc;     // F x 9
    ushort4* tbox;       // F: tile box (tx0, tx1, ty0, ty1); tx0 > tx1: the face leaves no fragment
    unsigned* tcount;    // tiles
    unsigned* toff;      // tiles + 1
    unsigned* cursor;    // tiles
    int* list;           // list_cap
    int tiles_x, tiles_y;
    size_t tiles, bytes;
};
Ws carve(const void* ws, int F, int H, int W, long long list_cap) {
    Ws w;
    w.tiles_x = (W + TILE - 1) / TILE, w.tiles_y = (H + TILE - 1) / TILE;
    w.tiles = (size_t)w.tiles_x * w.tiles_y;
    char* p = (char*)const_cast<void*>(ws);
    Carve cv;
    w.hdr = (Hdr*)(p + cv.take(sizeof(Hdr)));
    w.face_ndc = (float*)(p + cv.take((size_t)F * 9 * 4));
    w.tbox = (ushort4*)(p + cv.take((size_t)F * sizeof(ushort4)));
    w.tcount = (unsigned*)(p + cv.take(w.tiles * 4));
    w.toff = (unsigned*)(p + cv.take((w.tiles + 1) * 4));
    w.cursor = (unsigned*)(p + cv.take(w.tiles * 4));
    w.list = (int*)(p + cv.take((size_t)list_cap * 4));
    w.bytes = cv.off;
    return w;
}

// conservative range of (unflipped) pixel indices whose centre may lie in [lo, hi]: the analytic estimate widened by one pixel
// (k_vertex.inc's ndc_to_pix_range settles the exact range; here eval_frag tests the exact box per pixel anyway)
__device__ __forceinline__ void pix_range(float lo, float hi, const PixAxis& ax, int& p0, int& p1) {
    const float off = ax.offset;
    float flo = ((lo + off) * ax.s1 - off) / ax.range, fhi = ((hi + off) * ax.s1 - off) / ax.range;
    flo = fminf(fmaxf(flo, -2.0f), ax.s1 + 1.0f);
    fhi = fminf(fmaxf(fhi, -2.0f), ax.s1 + 1.0f);
    const int i0 = max(0, (int)floorf(flo) - 1), i1 = min(ax.S1 - 1, (int)ceilf(fhi) + 1);
    p0 = ax.S1 - 1 - i1;
    p1 = ax.S1 - 1 - i0;
}

__global__ __launch_bounds__(TPB) void k_rk_setup(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int F,
                                                  PixAxis ax, PixAxis ay, float sqrt_blur, int tiles_x, float* __restrict__ face_ndc,
                                                  ushort4* __restrict__ tbox, unsigned* tcount) {
    const int f = blockIdx.x * TPB + threadIdx.x;
    if (f >= F) return;
    int vi[3];
    bool valid = true;
    for (int k = 0; k < 3; k++) {
        vi[k] = faces[3 * (size_t)f + k];
        valid = valid && vi[k] >= 0 && vi[k] < V;
    }
    float fv[9];
    for (int k = 0; k < 3; k++)
        for (int q = 0; q < 3; q++) fv[3 * k + q] = valid ? verts[3 * (size_t)vi[k] + q] : 0.0f;
    for (int k = 0; k < 9; k++) face_ndc[9 * (size_t)f + k] = fv[k];
    const float zmax = fmaxf(fmaxf(fv[2], fv[5]), fv[8]), zmin = fminf(fminf(fv[2], fv[5]), fv[8]);
    const float farea = edge_fn(fv[0], fv[1], fv[3], fv[4], fv[6], fv[7]);
    // near plane: faces entirely nearer than it are culled, a face that straddles it is rasterised as its sub-triangles
    const bool near_cull = zmax < Z_CLIP;
    const bool clipped = !near_cull && zmin < Z_CLIP;
    valid = valid && !near_cull && !(zmax < 0.0f) && (clipped || !(farea <= K_EPS && farea >= -K_EPS));
    int x0 = 1, x1 = 0, y0 = 1, y1 = 0;
    if (valid) {
        float xlo = fminf(fminf(fv[0], fv[3]), fv[6]), xhi = fmaxf(fmaxf(fv[0], fv[3]), fv[6]);
        float ylo = fminf(fminf(fv[1], fv[4]), fv[7]), yhi = fmaxf(fmaxf(fv[1], fv[4]), fv[7]);
        if (clipped) {  // pixel box of the clipped polygon = union of the sub-triangles' boxes
            float t0[9], t1[9];
            const ClipGeom g = clip_subtris(fv, Z_CLIP, t0, t1);
            xlo = fminf(fminf(t0[0], t0[3]), t0[6]);
            xhi = fmaxf(fmaxf(t0[0], t0[3]), t0[6]);
            ylo = fminf(fminf(t0[1], t0[4]), t0[7]);
            yhi = fmaxf(fmaxf(t0[1], t0[4]), t0[7]);
            if (g.n == 2) {
                xlo = fminf(xlo, fminf(fminf(t1[0], t1[3]), t1[6]));
                xhi = fmaxf(xhi, fmaxf(fmaxf(t1[0], t1[3]), t1[6]));
                ylo = fminf(ylo, fminf(fminf(t1[1], t1[4]), t1[7]));
                yhi = fmaxf(yhi, fmaxf(fmaxf(t1[1], t1[4]), t1[7]));
            }
            valid = g.n > 0;
        }
        xlo -= sqrt_blur, xhi += sqrt_blur, ylo -= sqrt_blur, yhi += sqrt_blur;
        valid = valid && (xlo == xlo) && (xhi == xhi) && (ylo == ylo) && (yhi == yhi);  // a NaN vertex fails every box test
        if (valid) {
            pix_range(xlo, xhi, ax, x0, x1);
            pix_range(ylo, yhi, ay, y0, y1);
            valid = (x0 <= x1) && (y0 <= y1);
        }
    }
    ushort4 tb = make_ushort4(1, 0, 1, 0);
    if (valid) {
        tb = make_ushort4((unsigned short)(x0 / TILE), (unsigned short)(x1 / TILE), (unsigned short)(y0 / TILE), (unsigned short)(y1 / TILE));
        for (int ty = tb.z; ty <= tb.w; ty++)
            for (int tx = tb.x; tx <= tb.y; tx++) atomicAdd(&tcount[(size_t)ty * tiles_x + tx], 1u);
    }
    tbox[f] = tb;
}

// one workgroup: thread t owns tiles [t seg, (t + 1) seg)
__global__ __launch_bounds__(TPB) void k_rk_scan(const unsigned* __restrict__ tcount, unsigned* __restrict__ toff, unsigned* __restrict__ cursor,
                                                 long long tiles, long long list_cap, Hdr* hdr, int32_t* overflow) {
    __shared__ unsigned long long s_sum[TPB];
    const int t = threadIdx.x;
    const long long seg = (tiles + TPB - 1) / TPB;
    const long long b = min((long long)t * seg, tiles), e = min(b + seg, tiles);
    unsigned long long s = 0;
    for (long long i = b; i < e; i++) s += tcount[i];
    const unsigned long long before = block_exclusive_scan<TPB>(s, s_sum);
    const unsigned long long total = s_sum[TPB - 1];
    const bool over = total > (unsigned long long)list_cap;
    if (t == 0) {
        hdr->need = (long long)total;
        hdr->abort = over ? 1 : 0;
        hdr->pad = 0;
        *overflow = over ? FOHO_RASTK_OVER_LIST : 0;
    }
    if (over) return;
    unsigned run = (unsigned)before;
    for (long long i = b; i < e; i++) {
        toff[i] = run;
        cursor[i] = run;
        run += tcount[i];
    }
    if (t == TPB - 1) toff[tiles] = (unsigned)total;
}

__global__ __launch_bounds__(TPB) void k_rk_fill(const ushort4* __restrict__ tbox, int F, int tiles_x, unsigned* cursor, int* __restrict__ list,
                                                 const Hdr* __restrict__ hdr) {
    if (hdr->abort) return;
    const int f = blockIdx.x * TPB + threadIdx.x;
    if (f >= F) return;
    const ushort4 tb = tbox[f];
    for (int ty = tb.z; ty <= tb.w; ty++)
        for (int tx = tb.x; tx <= tb.y; tx++) list[atomicAdd(&cursor[(size_t)ty * tiles_x + tx], 1u)] = f;
}

// one triangle at one pixel centre, the oracle's tests (eval_frag) plus cull_backfaces (face_area < 0 on the triangle that is
// rasterised: a sub-triangle for a clipped face)
__device__ __forceinline__ bool eval_tri(const float* t, bool cull, float xf, float yf, float blur, float sqrt_blur, Frag& out) {
    if (cull && edge_fn(t[0], t[1], t[3], t[4], t[6], t[7]) < 0.0f) return false;
    return eval_frag<false>(t, xf, yf, blur, sqrt_blur, out);
}
// one face at one pixel centre.  sub: -1 the face itself, 0 / 1 the sub-triangle of a face cut by the near plane the fragment
// belongs to (barycentrics are the sub-triangle's).  With cull off this IS eval_frag_near (foho_common.h), the function the scatter
// rasteriser and its export call, so the neighbour rule -- a face with one vertex behind the plane gives a fragment from at most
// one of its two halves, the second only when strictly closer to its edges -- lives in one place; applied before insertion.
// With cull on, pytorch3d tests the area sign of the triangle that is RASTERISED, i.e. of each sub-triangle: a culled half is a
// half without a fragment, which is eval_frag_near's rule on a face whose culled half is absent -- the surviving half alone.
__device__ __forceinline__ bool eval_face(const float* fv, bool cull, float xf, float yf, float blur, float sqrt_blur, Frag& out, int& sub) {
    if (!cull) return eval_frag_near(fv, Z_CLIP, xf, yf, blur, sqrt_blur, out, sub);
    sub = -1;
    if (!(fminf(fminf(fv[2], fv[5]), fv[8]) < Z_CLIP)) return eval_tri(fv, true, xf, yf, blur, sqrt_blur, out);
    float t0[9], t1[9];
    const ClipGeom g = clip_subtris(fv, Z_CLIP, t0, t1);
    const bool back0 = edge_fn(t0[0], t0[1], t0[3], t0[4], t0[6], t0[7]) < 0.0f;
    const bool back1 = g.n == 2 && edge_fn(t1[0], t1[1], t1[3], t1[4], t1[6], t1[7]) < 0.0f;
    if (g.n == 0 || (back0 && (g.n == 1 || back1))) return false;
    if (!back0 && !back1) return eval_frag_near(fv, Z_CLIP, xf, yf, blur, sqrt_blur, out, sub);  // nothing culled: the shared rule
    sub = back0 ? 1 : 0;  // one half of a split face is culled: the other half alone
    return eval_frag<false>(back0 ? t1 : t0, xf, yf, blur, sqrt_blur, out);
}

// The selection loop and the column sort of one wave's tile (k_rk_select, k_rk_render_fwd / _bwd): the tile's faces [beg, end) of
// `list` stream through s_fv / s_id in chunks of CH, the lane keeps the K smallest keys of its pixel in its slab column
// (slab[slot * 64 + lane]) and sorts them ascending.  Every lane of the wave calls it (it holds barriers); a lane outside the image
// keeps nothing.  Returns the number of keys kept, cnt = the fragments the pixel received before the cut.
__device__ __forceinline__ int select_sort(unsigned long long* slab, float* s_fv, int* s_id, const float* __restrict__ face_ndc,
                                           const int* __restrict__ list, unsigned beg, unsigned end, int lane, bool in_img, int K, bool cull,
                                           float xf, float yf, float blur, float sqrt_blur, int& cnt) {
    int n = 0, imax = 0;
    cnt = 0;
    unsigned long long kmax = 0ull;
    for (unsigned c0 = beg; c0 < end; c0 += CH) {
        const int m = (int)min((unsigned)CH, end - c0);
        if (lane < m) {
            const int f = list[c0 + lane];
            s_id[lane] = f;
            for (int k = 0; k < 9; k++) s_fv[lane * 9 + k] = face_ndc[9 * (size_t)f + k];
        }
        __syncthreads();
        if (in_img) {
            for (int j = 0; j < m; j++) {
                float fv[9];
                for (int k = 0; k < 9; k++) fv[k] = s_fv[j * 9 + k];
                Frag fr;
                int sub;
                if (!eval_face(fv, cull, xf, yf, blur, sqrt_blur, fr, sub)) continue;
                // z >= 0 (pz < 0 leaves no fragment, -0 was canonicalised): the float's bits order as unsigned
                const unsigned long long key = ((unsigned long long)__float_as_uint(fr.z) << 32) | ((unsigned)s_id[j] << 1) | (unsigned)(sub == 1);
                cnt++;
                if (n < K) {
                    slab[n * 64 + lane] = key;
                    if (n == 0 || key > kmax) {
                        kmax = key;
                        imax = n;
                    }
                    n++;
                } else if (key < kmax) {  // replaces the farthest kept fragment; the new maximum by a scan of the column
                    slab[imax * 64 + lane] = key;
                    kmax = 0ull;
                    for (int i = 0; i < K; i++) {
                        const unsigned long long v = slab[i * 64 + lane];
                        if (v >= kmax) {
                            kmax = v;
                            imax = i;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    // the lane's column, ascending (insertion sort: columns are short, and nearly always far below K)
    for (int i = 1; i < n; i++) {
        const unsigned long long v = slab[i * 64 + lane];
        int j = i;
        while (j > 0) {
            const unsigned long long u = slab[(j - 1) * 64 + lane];
            if (!(u > v)) break;
            slab[j * 64 + lane] = u;
            j--;
        }
        slab[j * 64 + lane] = v;
    }
    return n;
}

// the fragment a kept key came from, evaluated again: its face id; fr.z is bitwise the key's high word.  BARY: b = its barycentrics,
// which refer to the UNCLIPPED face, like pytorch3d's
template <bool BARY>
__device__ __forceinline__ int eval_kept(unsigned long long key, const float* __restrict__ face_ndc, bool cull, float xf, float yf, float blur,
                                         float sqrt_blur, Frag& fr, float* b) {
    const int f = (int)((unsigned)(key & 0xffffffffull) >> 1);
    float fv[9];
    for (int q = 0; q < 9; q++) fv[q] = face_ndc[9 * (size_t)f + q];
    int sub;
    eval_face(fv, cull, xf, yf, blur, sqrt_blur, fr, sub);
    if (BARY) {
        b[0] = fr.c0, b[1] = fr.c1, b[2] = fr.c2;
        if (sub >= 0) subtri_bary_to_face(fv, Z_CLIP, sub, b);
    }
    return f;
}

template <int KCAP>
__global__ __launch_bounds__(64) void k_rk_select(const float* __restrict__ face_ndc, const unsigned* __restrict__ toff, const int* __restrict__ list,
                                                  const Hdr* __restrict__ hdr, int H, int W, int K, PixAxis ax, PixAxis ay, float blur,
                                                  float sqrt_blur, int cull, int tiles_x, int64_t* __restrict__ p2f, float* __restrict__ zbuf,
                                                  float* __restrict__ bary, float* __restrict__ dists, int32_t* __restrict__ counts) {
    __shared__ unsigned long long slab[KCAP * 64];
    __shared__ float s_fv[CH * 9];
    __shared__ int s_id[CH];
    if (hdr->abort) return;
    const int lane = threadIdx.x;
    const int tile = blockIdx.x;
    const int px = (tile % tiles_x) * TILE + (lane & (TILE - 1)), py = (tile / tiles_x) * TILE + (lane >> 3);
    const bool in_img = px < W && py < H;
    const float xf = pix_to_ndc(W - 1 - px, ax), yf = pix_to_ndc(H - 1 - py, ay);
    int cnt;
    const int n = select_sort(slab, s_fv, s_id, face_ndc, list, toff[tile], toff[tile + 1], lane, in_img, K, cull != 0, xf, yf, blur, sqrt_blur, cnt);
    if (!in_img) return;
    const size_t pix = (size_t)py * W + px;
    if (counts) counts[pix] = cnt;
    for (int k = 0; k < K; k++) {
        const size_t o = pix * (size_t)K + k;
        int64_t face = -1;
        float z = -1.0f, sd = -1.0f, b[3] = {-1.0f, -1.0f, -1.0f};
        if (k < n) {
            Frag fr;
            face = eval_kept<true>(slab[k * 64 + lane], face_ndc, cull != 0, xf, yf, blur, sqrt_blur, fr, b);
            z = fr.z;
            sd = fr.sdist;
        }
        p2f[o] = face;
        zbuf[o] = z;
        dists[o] = sd;
        bary[3 * o] = b[0];
        bary[3 * o + 1] = b[1];
        bary[3 * o + 2] = b[2];
    }
}

__global__ __launch_bounds__(TPB) void k_rk_bwd(const float* __restrict__ verts, const int32_t* __restrict__ faces, int V, int F, int H, int W,
                                                int K, const int64_t* __restrict__ p2f, const float* __restrict__ g_z, const float* __restrict__ g_b,
                                                const float* __restrict__ g_d, float* g_verts, float blur, float sqrt_blur) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= (size_t)H * W * K) return;
    const int64_t f = p2f[i];
    if (f < 0 || f >= F) return;
    int vi[3];
    for (int k = 0; k < 3; k++) {
        vi[k] = faces[3 * f + k];
        if (vi[k] < 0 || vi[k] >= V) return;
    }
    float fv[9], gv[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 3; k++)
        for (int q = 0; q < 3; q++) fv[3 * k + q] = verts[3 * (size_t)vi[k] + q];
    const size_t pix = i / (size_t)K;
    const int py = (int)(pix / W), px = (int)(pix % W);
    const float gc[3] = {g_b ? g_b[3 * i] : 0.f, g_b ? g_b[3 * i + 1] : 0.f, g_b ? g_b[3 * i + 2] : 0.f};
    eval_frag_near_bwd<true>(fv, Z_CLIP, blur, sqrt_blur, pix_to_ndc(W - 1 - px, W, H), pix_to_ndc(H - 1 - py, H, W), g_z ? g_z[i] : 0.f, gc,
                       g_d ? g_d[i] : 0.f, gv);
    for (int k = 0; k < 3; k++)
        for (int q = 0; q < 3; q++)
            if (gv[3 * k + q] != 0.f) atomicAdd(&g_verts[3 * (size_t)vi[k] + q], gv[3 * k + q]);
}

// setup, scan and fill: the tile lists of one frame into the workspace (foho_rastk_fwd, foho_rastk_render_fwd); false: the memset failed
bool bin_faces(const Ws& w, const float* verts_ndc, const int32_t* faces, int V, int F, const PixAxis& ax, const PixAxis& ay, float sqrt_blur,
               int64_t list_cap, int32_t* overflow, hipStream_t st) {
    if (hipMemsetAsync(w.tcount, 0, w.tiles * 4, st) != hipSuccess) return false;
    hipLaunchKernelGGL(k_rk_setup, dim3(blocks_for(F, TPB)), dim3(TPB), 0, st, verts_ndc, faces, V, F, ax, ay, sqrt_blur, w.tiles_x, w.face_ndc,
                       w.tbox, w.tcount);
    hipLaunchKernelGGL(k_rk_scan, dim3(1), dim3(TPB), 0, st, w.tcount, w.toff, w.cursor, (long long)w.tiles, (long long)list_cap, w.hdr, overflow);
    hipLaunchKernelGGL(k_rk_fill, dim3(blocks_for(F, TPB)), dim3(TPB), 0, st, w.tbox, F, w.tiles_x, w.cursor, w.list, w.hdr);
    return true;
}

bool dims_ok(int32_t V, int32_t F, int32_t H, int32_t W) {
    return V >= 1 && F >= 1 && F <= (1 << 30) && H >= 1 && W >= 1 && H <= 8192 && W <= 8192 && (size_t)H * W <= ((size_t)1 << 25);
}
bool k_ok(int32_t K) { return K >= 1 && K <= FOHO_RASTK_MAX_K; }
bool cap_ok(int64_t c) { return c >= 0 && c <= FOHO_RASTK_MAX_LIST; }

}  // namespace

FOHO_SIDE_ENTRY_POINTS(rastk, FOHO_RASTK_API, FOHO_RASTK_VERSION)

extern "C" {

FOHO_RASTK_API size_t foho_rastk_workspace_bytes(int32_t V, int32_t F, int32_t H, int32_t W, int32_t K, int64_t list_cap) {
    if (!dims_ok(V, F, H, W) || !k_ok(K) || !cap_ok(list_cap)) return 0;
    return carve(nullptr, F, H, W, list_cap).bytes;
}

FOHO_RASTK_API int foho_rastk_fwd(const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                                  float blur_radius, int32_t flags, int64_t* pix_to_face, float* zbuf, float* bary, float* dists,
                                  int32_t* counts, int32_t* overflow, int64_t list_cap, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    if (!verts_ndc || !faces || !pix_to_face || !zbuf || !bary || !dists || !overflow || !workspace) return fail(-1, "foho_rastk_fwd: null argument");
    if (!k_ok(K)) return fail(-1, "foho_rastk_fwd: K outside 1 .. 128");
    if (!dims_ok(V, F, H, W)) return fail(-1, "foho_rastk_fwd: V, F, H or W out of range");
    if (!cap_ok(list_cap)) return fail(-1, "foho_rastk_fwd: list_cap out of range");
    if (!(blur_radius >= 0.0f)) return fail(-1, "foho_rastk_fwd: negative blur radius");
    if (flags & ~FOHO_RASTK_CULL_BACKFACES) return fail(-1, "foho_rastk_fwd: unknown flag");
    const Ws w = carve(workspace, F, H, W, list_cap);
    if (workspace_bytes < w.bytes) return fail(-3, "foho_rastk_fwd: workspace too small (query foho_rastk_workspace_bytes)");
    const hipStream_t st = (hipStream_t)stream;
    const PixAxis ax = pix_axis(W, H), ay = pix_axis(H, W);
    const float sqrt_blur = sqrtf(blur_radius);
    const int cull = (flags & FOHO_RASTK_CULL_BACKFACES) ? 1 : 0;
    if (!bin_faces(w, verts_ndc, faces, V, F, ax, ay, sqrt_blur, list_cap, overflow, st)) return fail(-2, "foho_rastk_fwd: memset failed");
#define RK_SELECT(KCAP)                                                                                                                  \
    hipLaunchKernelGGL(k_rk_select<KCAP>, dim3((unsigned)w.tiles), dim3(64), 0, st, w.face_ndc, w.toff, w.list, w.hdr, H, W, K, ax, ay, \
                       blur_radius, sqrt_blur, cull, w.tiles_x, pix_to_face, zbuf, bary, dists, counts)
    // the slab is sized by K's class: 4, 16 or 64 KB of LDS per wave
    if (K <= 8) RK_SELECT(8);
    else if (K <= 32) RK_SELECT(32);
    else RK_SELECT(128);
#undef RK_SELECT
    return launched("foho_rastk_fwd");
}

FOHO_RASTK_API int foho_rastk_bwd(const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                                  const int64_t* pix_to_face, const float* grad_zbuf, const float* grad_bary, const float* grad_dists,
                                  float* grad_verts_ndc, float blur_radius, void* stream) {
    if (!verts_ndc || !faces || !pix_to_face || !grad_verts_ndc) return fail(-1, "foho_rastk_bwd: null argument");
    if (!k_ok(K)) return fail(-1, "foho_rastk_bwd: K outside 1 .. 128");
    if (!dims_ok(V, F, H, W)) return fail(-1, "foho_rastk_bwd: V, F, H or W out of range");
    if (!(blur_radius >= 0.0f)) return fail(-1, "foho_rastk_bwd: negative blur radius");
    hipLaunchKernelGGL(k_rk_bwd, dim3(blocks_for((size_t)H * W * K, TPB)), dim3(TPB), 0, (hipStream_t)stream, verts_ndc, faces, V, F, H, W, K,
                       pix_to_face, grad_zbuf, grad_bary, grad_dists, grad_verts_ndc, blur_radius, sqrtf(blur_radius));
    return launched("foho_rastk_bwd");
}

}  // extern "C"

#include "rastk_blend.inc"   // foho_rastk_blend_fwd / _bwd
#include "rastk_render.inc"  // foho_rastk_render_fwd / _bwd
