// k_topo.inc -- topology tables of a packed hand + object mesh, built on the device for a mesh whose connectivity
// changes every iteration (the FlexiCubes output, pipelines.py:1393 / 1509).
//
// The step needs (a) vertex -> incident (face << 2 | corner) lists ordered corner-major then by face id -- the
// accumulation order of pytorch3d's three index_add calls in verts_normals_packed (PL:83) -- and (b) vertex ->
// neighbour lists over the unique undirected edges of the OBJECT mesh (Meshes.edges_packed / mesh_edge_loss, PL:1575).
// For a closed, consistently oriented 2-manifold (what dual marching cubes emits; the MANO surface with its wrist cap)
// (b) follows from (a): around a vertex every neighbour is the "next" vertex of exactly one incident face, the
// neighbour list has the length -- and shares the offsets -- of the incidence list, and the number of unique edges is
// 3 F / 2.  Vertices flagged as object vertices are checked; anything else (a duplicate neighbour, an open fan, a
// valence > TOPO_MAXVAL) raises a flag and the caller falls back to the general sort-based host / torch path.
//
// Two entry points build them: foho_topology_tables (here) for a mesh of exactly V vertices and F faces, and capacity mode's
// foho_object_update (k_object.inc, included after this file) for a batch of capacity-sized slots whose counts live on the
// device.  Both count, scan, fill and finish; the per-vertex work of the last kernel -- the sorts and the check -- is ONE device
// function, topo_vertex, under the two thin kernels k_topo_finish and k_topo_finish_b, and both carve their workspace with
// carve_topo and scan with topo_scan (two launches).
//
//   k_topo_count   per (face, corner): histogram of the vertex valences
//   topo_scan      exclusive prefix sum -> list offsets (k_flexi.inc's scan kernels)
//   k_topo_fill    per (face, corner): append to the vertex's list (atomic cursor; order fixed by the next kernel)
//   k_topo_finish  per vertex: topo_vertex in place; the closing offset; one flag word

constexpr int TOPO_MAXVAL = 48;                            // longest list served
constexpr int TOPO_FAST = 16;                              // longest list kept in registers
constexpr int TOPO_TPB = 64;                               // threads (= vertices) per workgroup of the two finish kernels
constexpr int TOPO_LDS_STRIDE = TOPO_MAXVAL + 1;           // words between two threads' LDS lists: odd, so conflict free
constexpr int TOPO_LDS_LIST = TOPO_TPB * TOPO_LDS_STRIDE;  // one list per thread; three of them: 37632 bytes per workgroup

__global__ void k_set_i32(int32_t* p, int32_t v) { *p = v; }

__global__ __launch_bounds__(256) void k_topo_count(const int32_t* faces, int F, int32_t* cnt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < 3 * F) atomicAdd(&cnt[faces[t]], 1);
}

__global__ __launch_bounds__(256) void k_topo_fill(const int32_t* faces, int F, const int32_t* inc_off, int32_t* cursor,
                                                   int32_t* inc_fc) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * F) return;
    const int v = faces[t], face = t / 3, corner = t % 3;
    const int pos = inc_off[v] + atomicAdd(&cursor[v], 1);
    inc_fc[pos] = (face << 2) | corner;
}

// insertion sort of a short LDS list, ascending by key(entry)
template <class Key>
__device__ __forceinline__ void topo_sort(int* a, int n, Key key) {
    for (int i = 1; i < n; i++) {
        const int x = a[i];
        const auto kx = key(x);
        int b = i - 1;
        while (b >= 0) {
            const int y = a[b];
            if (key(y) <= kx) break;
            a[b + 1] = y;
            b--;
        }
        a[b + 1] = x;
    }
}

// ---- the per-vertex core of k_topo_finish and k_topo_finish_b.  src[e0 .. e0 + n) = the vertex's n (>= 1) unsorted (face << 2 | corner)
// entries; its lists go to the same range of inc_dst / nbr_dst / pair_dst.  Orders the list by (corner, face), derives the next vertex
// (= neighbour) and the previous vertex of every incident face, sorts the neighbours ascending and -- when `check` -- verifies that no
// neighbour repeats (more than two faces on an edge) and that every previous vertex is a neighbour too (a closed fan).  Returns 0 or one of
constexpr int TOPO_OVERFLOW = 1;      // more than TOPO_MAXVAL incident faces: nothing written
constexpr int TOPO_NOT_MANIFOLD = 2;  // the check failed (the lists are written all the same)
// What is written is decided at compile time: inc_dst always (it may be `src` itself: every read of the list precedes the first write);
// NBR: the neighbour list, and only then `check` counts; PAIR: the (v0, v1, v2, corner) records of the normal backward (pack_pair).
// n <= TOPO_FAST: the list stays in registers and is ordered by COUNTING -- rank = number of smaller keys, all compile-time indexed, no
// dependent chain.  Longer lists: insertion sorts on the thread's three LDS lists e, d, pv (TOPO_LDS_STRIDE words between threads;
// run-time indexed private arrays would live in scratch memory).  F = the multiplier of the (corner, face) sort key.
template <bool NBR, bool PAIR>
__device__ __forceinline__ int topo_vertex(const int32_t* faces, const int32_t* src, int e0, int n, int F, bool check, int32_t* inc_dst,
                                           int32_t* nbr_dst, unsigned long long* pair_dst, int* e, int* d, int* pv) {
    static_assert(NBR || !PAIR, "the pair table comes with the neighbour lists");
    if (n > TOPO_MAXVAL) return TOPO_OVERFLOW;
    int bad = 0;
    if (n <= TOPO_FAST && F < (1 << 28)) {  // (the 32-bit key below holds face ids up to 2^28)
        int x[TOPO_FAST], f[TOPO_FAST][3];
#pragma unroll
        for (int u = 0; u < TOPO_FAST; u++) x[u] = src[e0 + min(u, n - 1)];
#pragma unroll
        for (int u = 0; u < TOPO_FAST; u++)
            for (int k = 0; k < 3; k++) f[u][k] = faces[3 * (size_t)(x[u] >> 2) + k];
        unsigned key[TOPO_FAST];
        int nx[TOPO_FAST];
#pragma unroll
        for (int u = 0; u < TOPO_FAST; u++) {
            const int corner = x[u] & 3;
            key[u] = (u < n) ? (((unsigned)corner << 28) | (unsigned)(x[u] >> 2)) : 0xffffffffu;  // (corner, face): unique
            nx[u] = (u < n) ? ((corner == 0) ? f[u][1] : ((corner == 1) ? f[u][2] : f[u][0])) : 0x7fffffff;
        }
#pragma unroll
        for (int u = 0; u < TOPO_FAST; u++) {
            // (the previous vertex here, not in a list of its own: 16 registers less over the ranking)
            const int corner = x[u] & 3, prev = (corner == 0) ? f[u][2] : ((corner == 1) ? f[u][0] : f[u][1]);
            int rk = 0, rd = 0, dup = 0, found = 0;
#pragma unroll
            for (int j = 0; j < TOPO_FAST; j++) {
                rk += (key[j] < key[u]) ? 1 : 0;
                rd += (nx[j] < nx[u] || (nx[j] == nx[u] && j < u)) ? 1 : 0;
                dup |= (j < u && nx[j] == nx[u]) ? 1 : 0;
                found |= (nx[j] == prev) ? 1 : 0;
            }
            if (u < n) {
                inc_dst[e0 + rk] = x[u];
                if constexpr (PAIR) pair_dst[e0 + rk] = pack_pair(f[u][0], f[u][1], f[u][2], corner);
                if constexpr (NBR) {
                    nbr_dst[e0 + rd] = nx[u];
                    if (check) bad |= dup | (found ^ 1);
                }
            }
        }
        return bad ? TOPO_NOT_MANIFOLD : 0;
    }
    // the list, eight loads in flight at a time
    for (int base = 0; base < n; base += 8) {
        int x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = src[e0 + min(base + u, n - 1)];
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (base + u < n) e[base + u] = x[u];
    }
    topo_sort(e, n, [F](int x) { return (long long)(x & 3) * F + (x >> 2); });
    if constexpr (!NBR) {
        for (int q = 0; q < n; q++) inc_dst[e0 + q] = e[q];
        return 0;
    } else {
        // the faces of the list, 24 loads in flight at a time: pair record, next vertex (neighbour), previous vertex
        for (int base = 0; base < n; base += 8) {
            int x[8], f[8][3];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = e[min(base + u, n - 1)];
#pragma unroll
            for (int u = 0; u < 8; u++)
                for (int k = 0; k < 3; k++) f[u][k] = faces[3 * (size_t)(x[u] >> 2) + k];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (base + u >= n) break;
                const int corner = x[u] & 3;
                inc_dst[e0 + base + u] = x[u];
                if constexpr (PAIR) pair_dst[e0 + base + u] = pack_pair(f[u][0], f[u][1], f[u][2], corner);
                d[base + u] = (corner == 0) ? f[u][1] : ((corner == 1) ? f[u][2] : f[u][0]);
                pv[base + u] = (corner == 0) ? f[u][2] : ((corner == 1) ? f[u][0] : f[u][1]);
            }
        }
        topo_sort(d, n, [](int x) { return x; });
        for (int q = 0; q < n; q++) nbr_dst[e0 + q] = d[q];
        if (check) {
            for (int q = 1; q < n; q++) bad |= (d[q] == d[q - 1]);
            for (int q = 0; q < n && !bad; q++) {
                const int p = pv[q];
                bool found = false;
                for (int r = 0; r < n; r++) found = found || (d[r] == p);
                bad = !found;
            }
        }
        return bad ? TOPO_NOT_MANIFOLD : 0;
    }
}

// exact-size tables, sorted in place.  NBR = false (obj_flag == NULL, the target-map render): incidence lists only, no check.
// flag: bit 0 = a valence above TOPO_MAXVAL, bit 1 = a checked vertex is not manifold.
template <bool NBR>
__global__ __launch_bounds__(TOPO_TPB) void k_topo_finish(const int32_t* faces, int V, int F, const uint8_t* obj_flag, int32_t* inc_off,
                                                          int32_t* inc_fc, int32_t* nbr_idx, int32_t* flag) {
    __shared__ int s_e[TOPO_LDS_LIST], s_d[TOPO_LDS_LIST], s_p[TOPO_LDS_LIST];
    const int v = blockIdx.x * TOPO_TPB + threadIdx.x, t = threadIdx.x * TOPO_LDS_STRIDE;
    if (v > V) return;
    if (v == V) {  // closing offset
        inc_off[V] = 3 * F;
        return;
    }
    const int e0 = inc_off[v], e1 = (v + 1 < V) ? inc_off[v + 1] : 3 * F;  // inc_off[V] is being written by the thread above
    const int n = e1 - e0;
    if (n <= 0) return;
    const int st = topo_vertex<NBR, false>(faces, inc_fc, e0, n, F, NBR && obj_flag[v], inc_fc, nbr_idx, nullptr, s_e + t, s_d + t, s_p + t);
    if (st) atomicOr(flag, st);
}

// ---- workspace of both entry points: valence counters and fill cursors of `items` vertices (zero when the count starts), the scan's
// block sums, a tail of the caller's
struct TopoWs {
    int32_t *cnt, *cursor, *bsum;
    char* tail;
    int nb;
    size_t counters, total;  // bytes of cnt + cursor; of everything
};
static TopoWs carve_topo(void* ws, size_t items, size_t tail_bytes) {
    char* p = (char*)ws;
    Carve cv;
    TopoWs w;
    w.nb = (int)((items + FX_ITEMS - 1) / FX_ITEMS);
    w.cnt = (int32_t*)(p + cv.take(items * 4));
    w.cursor = (int32_t*)(p + cv.take(items * 4));
    w.counters = cv.off;
    w.bsum = (int32_t*)(p + cv.take(((size_t)w.nb + 1) * 4));
    w.tail = p + cv.take(tail_bytes);
    w.total = cv.off;
    return w;
}
// valences -> list offsets: the block sums, then every workgroup adds up the sums in front of it (k_flexi.inc)
static int topo_scan(const TopoWs& w, size_t items, int32_t* inc_off, hipStream_t stream) {
    hipLaunchKernelGGL(k_scan_sums, dim3(w.nb), dim3(256), 0, stream, w.cnt, items, w.bsum);
    CHECK_LAUNCH("k_scan_sums");
    hipLaunchKernelGGL(k_scan_apply_p, dim3(w.nb), dim3(256), 0, stream, w.cnt, items, w.bsum, inc_off);
    CHECK_LAUNCH("k_scan_apply_p");
    return FOHO_OK;
}

// the tail: 16 reserved bytes (the grand total of the former three-launch scan; unused, kept so that the size callers allocate stays)
static TopoWs carve_tables(void* ws, int32_t V) { return carve_topo(ws, (size_t)V, 16); }

extern "C" size_t foho_topology_workspace_bytes(int32_t V) { return V < 1 ? 0 : carve_tables(nullptr, V).total; }

extern "C" int foho_topology_tables(const int32_t* faces, int32_t V, int32_t F, const uint8_t* obj_flag, int32_t* inc_off,
                                    int32_t* inc_fc, int32_t* nbr_idx, int32_t* flag, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
    if (!faces || !inc_off || !inc_fc || !flag || V < 1 || F < 1 || (obj_flag && !nbr_idx)) {
        foho_set_error("foho_topology_tables: bad argument");
        return FOHO_ERR_BAD_ARG;
    }
    if (!workspace || workspace_bytes < foho_topology_workspace_bytes(V)) {
        foho_set_error("foho_topology_tables: workspace too small (query foho_topology_workspace_bytes)");
        return FOHO_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const TopoWs w = carve_tables(workspace, V);
    const size_t n16 = w.counters / 16;
    hipLaunchKernelGGL(k_zero, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 1024)), dim3(256), 0, stream, (uint4*)workspace, n16);
    CHECK_LAUNCH("k_zero");
    hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, stream, flag, 0);
    CHECK_LAUNCH("k_set_i32");
    hipLaunchKernelGGL(k_topo_count, dim3((3 * F + 255) / 256), dim3(256), 0, stream, faces, F, w.cnt);
    CHECK_LAUNCH("k_topo_count");
    if (const int rc = topo_scan(w, (size_t)V, inc_off, stream)) return rc;
    hipLaunchKernelGGL(k_topo_fill, dim3((3 * F + 255) / 256), dim3(256), 0, stream, faces, F, inc_off, w.cursor, inc_fc);
    CHECK_LAUNCH("k_topo_fill");
    const dim3 grid(V / TOPO_TPB + 1);  // V + 1 threads: the last one writes the closing offset
    if (obj_flag) hipLaunchKernelGGL(k_topo_finish<true>, grid, dim3(TOPO_TPB), 0, stream, faces, V, F, obj_flag, inc_off, inc_fc, nbr_idx, flag);
    else hipLaunchKernelGGL(k_topo_finish<false>, grid, dim3(TOPO_TPB), 0, stream, faces, V, F, obj_flag, inc_off, inc_fc, nbr_idx, flag);
    CHECK_LAUNCH("k_topo_finish");
    return FOHO_OK;
}
