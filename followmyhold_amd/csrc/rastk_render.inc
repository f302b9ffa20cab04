// rastk_render.inc -- foho_rastk_render_fwd / _bwd (foho_rastk.h): mesh -> blended image and grad_out -> vertex / attribute gradients
// without the (H,W,K) planes.  Included by foho_rastk.hip behind rastk_blend.inc.  DESIGN.md section 3D.
//
// The bins are foho_rastk_fwd's (bin_faces: setup, scan, fill; the same workspace).  Then one wave per 8x8 tile runs k_rk_select's
// selection loop and column sort (select_sort), and the lane blends its own sorted column where it lies, in LDS: the sweeps of
// rastk_blend.inc over SlabFrags in place of the planes.
//   forward   sweep A from the keys alone (z is the key's high word, bitwise the zbuf entry); sweep B evaluates each kept fragment
//             once from its key (eval_kept, as k_rk_select's write-out) for the distance and the barycentrics
//   backward  the workspace the forward left (face_ndc, toff, list: no second binning); selection, sort, sweeps A and B again; sweep C
//             hands each fragment's g_z, g_bary, g_dist to eval_frag_near_bwd, the call k_rk_bwd makes, and adds to the vertices
// Nothing K-sized lives in registers or scratch; a fragment is evaluated again in every sweep that needs more than its depth (one
// code path for every K: the 64 KB slab of the K <= 128 class leaves no LDS to cache them in).  The slab is dynamic LDS, so K's class
// is a launch parameter and the instances are (D, unit weights) and alpha only.
namespace {

struct SlabFrags {
    const unsigned long long* col;  // slab + lane: slot k at col[k * 64]
    int n;
    const float* face_ndc;
    float xf, yf, blur, sqrt_blur;
    bool cull;
    __device__ __forceinline__ bool has(int k) const { return k < n; }
    __device__ __forceinline__ float z(int k) const { return __uint_as_float((unsigned)(col[k * 64] >> 32)); }
    __device__ __forceinline__ int64_t face(int k) const { return (int64_t)((unsigned)(col[k * 64] & 0xffffffffull) >> 1); }
    template <bool BARY>
    __device__ __forceinline__ void shade(int k, float& d, float* b) const {
        Frag fr;
        eval_kept<BARY>(col[k * 64], face_ndc, cull, xf, yf, blur, sqrt_blur, fr, b);
        d = fr.sdist;
    }
};

// sweep C's gradients of one fragment -> its three vertices (float atomicAdd), through the per-fragment derivative of k_rk_bwd
struct VertexSink {
    const float* face_ndc;
    const int32_t* faces;
    float* g_verts;  // NULL: not wanted
    int V;
    float xf, yf, blur, sqrt_blur;
    __device__ __forceinline__ void emit(int, int64_t f, float gz, const float* gb, float gd) const {
        if (!g_verts) return;
        int vi[3];
        for (int k = 0; k < 3; k++) {
            vi[k] = faces[3 * f + k];
            if (vi[k] < 0 || vi[k] >= V) return;
        }
        float fv[9], gv[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < 9; q++) fv[q] = face_ndc[9 * (size_t)f + q];
        eval_frag_near_bwd<true>(fv, Z_CLIP, blur, sqrt_blur, xf, yf, gz, gb, gd, gv);
        for (int k = 0; k < 3; k++)
            for (int q = 0; q < 3; q++)
                if (gv[3 * k + q] != 0.f) atomicAdd(&g_verts[3 * (size_t)vi[k] + q], gv[3 * k + q]);
    }
};

struct RenderGeom {
    const float* face_ndc;
    const unsigned* toff;
    const int* list;
    const Hdr* hdr;
    int H, W, K, cull, tiles_x;
    PixAxis ax, ay;
    float blur, sqrt_blur;
};

// the wave's tile: selection and sort into the slab; false for a lane outside the image
#define RK_RENDER_HEAD                                                                                                                       \
    extern __shared__ __attribute__((aligned(16))) unsigned long long slab[]; /* K's class x 64 keys */                                      \
    __shared__ float s_fv[CH * 9];                                                                                                           \
    __shared__ int s_id[CH];                                                                                                                 \
    if (g.hdr->abort) return;                                                                                                                \
    const int lane = threadIdx.x, tile = blockIdx.x;                                                                                         \
    const int px = (tile % g.tiles_x) * TILE + (lane & (TILE - 1)), py = (tile / g.tiles_x) * TILE + (lane >> 3);                            \
    const bool in_img = px < g.W && py < g.H;                                                                                                \
    const float xf = pix_to_ndc(g.W - 1 - px, g.ax), yf = pix_to_ndc(g.H - 1 - py, g.ay);                                                    \
    int cnt;                                                                                                                                 \
    const int n = select_sort(slab, s_fv, s_id, g.face_ndc, g.list, g.toff[tile], g.toff[tile + 1], lane, in_img, g.K, g.cull != 0, xf, yf, \
                              g.blur, g.sqrt_blur, cnt);                                                                                     \
    if (!in_img) return;                                                                                                                     \
    const size_t pix = (size_t)py * g.W + px;                                                                                                \
    const SlabFrags fr = {slab + lane, n, g.face_ndc, xf, yf, g.blur, g.sqrt_blur, g.cull != 0}

template <int D, bool UNIT, bool ALPHA>
__global__ __launch_bounds__(64) void k_rk_render_fwd(RenderGeom g, const float* __restrict__ attr, BlendCfg c, float* __restrict__ out,
                                                      int32_t* __restrict__ counts) {
    RK_RENDER_HEAD;
    if (counts) counts[pix] = cnt;
    if (ALPHA) {
        QProd pr;
        alpha_prod(fr, c.sigma, pr);
        out[pix] = 1.0f - pr.full();
    } else {
        write_pixel<D>(pixel_sums<D, UNIT>(fr, attr, c), c, out + pix * (D + 1));
    }
}

template <int D, bool UNIT, bool ALPHA>
__global__ __launch_bounds__(64) void k_rk_render_bwd(RenderGeom g, const int32_t* __restrict__ faces, int V, const float* __restrict__ attr,
                                                      BlendCfg c, const float* __restrict__ g_out, float* g_verts, float* g_attr) {
    RK_RENDER_HEAD;
    if (n == 0) return;  // no fragment: nothing depends on the mesh
    const VertexSink sink = {g.face_ndc, faces, g_verts, V, xf, yf, g.blur, g.sqrt_blur};
    if (ALPHA) {
        QProd pr;
        alpha_prod(fr, c.sigma, pr);
        alpha_grads(fr, n, pr, c.sigma, g_out[pix], sink);
    } else {
        pixel_grads<D, UNIT>(fr, pixel_sums<D, UNIT>(fr, attr, c), attr, c, g_out + pix * (D + 1), sink, g_attr);
    }
}
#undef RK_RENDER_HEAD

// the checks both entry points share: foho_rastk_fwd's and the blend's; 0 or the refusal's status
int render_args(const char* fn, const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                float blur_radius, int32_t raster_flags, const float* attr, int32_t D, float sigma, float gamma, float znear, float zfar,
                const float* background, int32_t blend_flags, int64_t list_cap, const void* workspace, size_t workspace_bytes, BlendCfg& c, Ws& w,
                RenderGeom& g) {
    const std::string who = std::string(fn) + ": ";
    if (!k_ok(K)) return fail(-1, who + "K outside 1 .. 128");
    if (!dims_ok(V, F, H, W)) return fail(-1, who + "V, F, H or W out of range");
    if (!cap_ok(list_cap)) return fail(-1, who + "list_cap out of range");
    if (!(blur_radius >= 0.0f)) return fail(-1, who + "negative blur radius");
    if (raster_flags & ~FOHO_RASTK_CULL_BACKFACES) return fail(-1, who + "unknown flag (raster_flags)");
    const int bad = blend_scalars(who, F, H, W, K, D, sigma, gamma, znear, zfar, blend_flags);
    if (bad) return bad;
    const bool alpha = blend_flags & FOHO_RASTK_BLEND_ALPHA_ONLY;
    if (!verts_ndc || !faces || !workspace || (!alpha && (!attr || !background))) return fail(-1, who + "null argument");
    w = carve(workspace, F, H, W, list_cap);
    if (workspace_bytes < w.bytes) return fail(-3, who + "workspace too small (query foho_rastk_workspace_bytes)");
    blend_cfg(c, F, H, W, K, D, sigma, gamma, znear, zfar, background, blend_flags);
    g.face_ndc = w.face_ndc, g.toff = w.toff, g.list = w.list, g.hdr = w.hdr;
    g.H = H, g.W = W, g.K = K, g.cull = (raster_flags & FOHO_RASTK_CULL_BACKFACES) ? 1 : 0, g.tiles_x = w.tiles_x;
    g.ax = pix_axis(W, H), g.ay = pix_axis(H, W);
    g.blur = blur_radius, g.sqrt_blur = sqrtf(blur_radius);
    return 0;
}

// one instance per (D, unit weights) and one for alpha only; the slab's bytes by K's class: 4, 16 or 64 KB of LDS per wave
#define RK_RENDER_DISPATCH(KERNEL, ...)                                                                                \
    do {                                                                                                               \
        const dim3 grid((unsigned)w.tiles), block(64);                                                                 \
        const size_t lds = (size_t)(K <= 8 ? 8 : K <= 32 ? 32 : 128) * 64 * sizeof(unsigned long long);                \
        const hipStream_t st = (hipStream_t)stream;                                                                    \
        const bool unit = blend_flags & FOHO_RASTK_BLEND_UNIT_BARY;                                                    \
        switch ((blend_flags & FOHO_RASTK_BLEND_ALPHA_ONLY) ? 0 : D * 2 + (unit ? 1 : 0)) {                            \
            case 0: hipLaunchKernelGGL((KERNEL<1, true, true>), grid, block, lds, st, __VA_ARGS__); break;            \
            case 2: hipLaunchKernelGGL((KERNEL<1, false, false>), grid, block, lds, st, __VA_ARGS__); break;          \
            case 3: hipLaunchKernelGGL((KERNEL<1, true, false>), grid, block, lds, st, __VA_ARGS__); break;           \
            case 4: hipLaunchKernelGGL((KERNEL<2, false, false>), grid, block, lds, st, __VA_ARGS__); break;          \
            case 5: hipLaunchKernelGGL((KERNEL<2, true, false>), grid, block, lds, st, __VA_ARGS__); break;           \
            case 6: hipLaunchKernelGGL((KERNEL<3, false, false>), grid, block, lds, st, __VA_ARGS__); break;          \
            case 7: hipLaunchKernelGGL((KERNEL<3, true, false>), grid, block, lds, st, __VA_ARGS__); break;           \
            case 8: hipLaunchKernelGGL((KERNEL<4, false, false>), grid, block, lds, st, __VA_ARGS__); break;          \
            default: hipLaunchKernelGGL((KERNEL<4, true, false>), grid, block, lds, st, __VA_ARGS__); break;          \
        }                                                                                                              \
    } while (0)

}  // namespace

extern "C" {

FOHO_RASTK_API int foho_rastk_render_fwd(const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                                         float blur_radius, int32_t raster_flags, const float* face_attr, int32_t D, float sigma, float gamma,
                                         float znear, float zfar, const float* background, int32_t blend_flags, float* out, int32_t* counts,
                                         int32_t* overflow, int64_t list_cap, void* workspace, size_t workspace_bytes, void* stream) {
    BlendCfg c;
    Ws w;
    RenderGeom g;
    const int bad = render_args("foho_rastk_render_fwd", verts_ndc, faces, V, F, H, W, K, blur_radius, raster_flags, face_attr, D, sigma, gamma,
                                znear, zfar, background, blend_flags, list_cap, workspace, workspace_bytes, c, w, g);
    if (bad) return bad;
    if (!out || !overflow) return fail(-1, "foho_rastk_render_fwd: null argument");
    if (!bin_faces(w, verts_ndc, faces, V, F, g.ax, g.ay, g.sqrt_blur, list_cap, overflow, (hipStream_t)stream))
        return fail(-2, "foho_rastk_render_fwd: memset failed");
    RK_RENDER_DISPATCH(k_rk_render_fwd, g, face_attr, c, out, counts);
    return launched("foho_rastk_render_fwd");
}

FOHO_RASTK_API int foho_rastk_render_bwd(const float* verts_ndc, const int32_t* faces, int32_t V, int32_t F, int32_t H, int32_t W, int32_t K,
                                         float blur_radius, int32_t raster_flags, const float* face_attr, int32_t D, float sigma, float gamma,
                                         float znear, float zfar, const float* background, int32_t blend_flags, const float* grad_out,
                                         float* grad_verts_ndc, float* grad_face_attr, int64_t list_cap, const void* workspace,
                                         size_t workspace_bytes, void* stream) {
    BlendCfg c;
    Ws w;
    RenderGeom g;
    const int bad = render_args("foho_rastk_render_bwd", verts_ndc, faces, V, F, H, W, K, blur_radius, raster_flags, face_attr, D, sigma, gamma,
                                znear, zfar, background, blend_flags, list_cap, workspace, workspace_bytes, c, w, g);
    if (bad) return bad;
    if (!grad_out) return fail(-1, "foho_rastk_render_bwd: null argument");
    if (blend_flags & FOHO_RASTK_BLEND_ALPHA_ONLY) grad_face_attr = nullptr;  // alpha depends on the distances alone
    if (!grad_verts_ndc && !grad_face_attr) return 0;
    RK_RENDER_DISPATCH(k_rk_render_bwd, g, faces, V, face_attr, c, grad_out, grad_verts_ndc, grad_face_attr);
    return launched("foho_rastk_render_bwd");
}

}  // extern "C"
#undef RK_RENDER_DISPATCH
