// k_object.inc -- CAPACITY MODE: the object mesh changes vertex count, face count and connectivity every iteration
// (the FlexiCubes output of the current latent, pipelines.py:1393 / 1509) and nothing of that may cost a host round trip.
//
// The caller sizes every buffer for a per-image CAPACITY (dims.Vo_max / Fo_max, image b's object slots start at
// images[b].v_off + Vh / f_off + Fh); the ACTUAL counts of an iteration live in device memory only: foho_flexi_fwd leaves
// them in `counts`, foho_object_update copies them into the device-resident foho_image records, and every kernel of the
// step takes its bounds from those records.  Grids are sized from the capacities; surplus workgroups leave at once.
// foho_flexi_fwd -> foho_object_update -> foho_step_run(FOHO_STAGE_STEP) -> foho_flexi_bwd is therefore a fixed launch
// sequence over fixed addresses: ONE hipGraph replay per iteration (engine.SdfObjective).
//
//   k_object_adopt    per image: counts -> image record (Vo, Fo, n_edges = 3 Fo / 2; capacity overflow -> empty object +
//                     flag bit 4; odd face count -> empty object + flag bit 5), int64 local face ids -> int32 global ids behind the hand's faces, valence histogram of
//                     all valid (face, corner) pairs, clears the AABB keys
//   topo_scan         valences -> list offsets (k_topo.inc; 2 launches)
//   k_object_fill     per (face, corner): append to the vertex's TEMPORARY list (atomic cursor; order fixed by the next kernel);
//                     extra workgroups: AABB of the new input meshes (centre of the similarity transform, PL:111)
//   k_topo_finish_b   per vertex: k_topo.inc's topo_vertex -- the core it shares with the exact-size k_topo_finish -- writing the
//                     ordered list, the neighbour list and the (vertex, face) pairs of the normal backward (what k_pair_table
//                     writes on the exact-size path); manifold check -> flag bit 5 of the owning image; hands the counters back zeroed

__global__ __launch_bounds__(256) void k_object_adopt(Ctx c, foho_image* img_rw, int32_t* faces_rw, const int32_t* counts,
                                                      const int64_t* obj_faces, int verts_cap, int faces_cap, int32_t* cnt) {
    const int b = blockIdx.y;
    const int v_off = img_rw[b].v_off, Vh = img_rw[b].Vh, f_off = img_rw[b].f_off, Fh = img_rw[b].Fh;
    int nv = counts[3 * b], nf = counts[3 * b + 1];
    // two different failures: the iso-surface does not fit the slots (bit 4: the host enlarges the capacity), or its face
    // count is odd -- no closed 2-manifold has one -- (bit 5: the host takes the exact-size path, the capacity is fine)
    const bool over = counts[3 * b + 2] != 0 || nv < 0 || nf < 0 || nv > verts_cap || nf > faces_cap;
    const bool odd = !over && (nf & 1);
    const bool bad = over || odd;
    if (bad) nv = nf = 0;  // keep the step well defined
    const int64_t* src = obj_faces + (size_t)b * faces_cap * 3;
    int32_t* dst = faces_rw + 3 * (size_t)(f_off + Fh);
    const int shift = v_off + Vh;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < 3 * nf; j += gridDim.x * 256) {
        const int v = (int32_t)src[j] + shift;
        dst[j] = v;
        atomicAdd(&cnt[v], 1);
    }
    const int32_t* hf = faces_rw + 3 * (size_t)f_off;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < 3 * Fh; j += gridDim.x * 256) atomicAdd(&cnt[hf[j]], 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        img_rw[b].Vo = nv;
        img_rw[b].Fo = nf;
        img_rw[b].n_edges = 3 * nf / 2;
        if (bad) atomicOr(&c.flags[b], over ? 16 : 32);
        else if (nv == 0 || nf == 0) atomicOr(&c.flags[b], 64);  // empty iso-surface: the reference skips the iteration (PL:1511-1513)
        for (int m = 0; m < 2; m++)
            for (int a = 0; a < 3; a++) c.mesh_info[2 * b + m].kmin_inv[a] = c.mesh_info[2 * b + m].kmax[a] = 0ull;
    }
}

// grid (fgrid + nbh + nbo, B): list fill for the first fgrid workgroups of a row, AABB role for the rest
__global__ __launch_bounds__(256) void k_object_fill(Ctx c, BboxCfg bc, int fgrid, const int32_t* inc_off, int32_t* cursor,
                                                     int32_t* inc_tmp) {
    if ((int)blockIdx.x >= fgrid) return bbox_role(c, bc, (int)blockIdx.x - fgrid, (int)blockIdx.y);
    const foho_image im = c.img[blockIdx.y];
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * (im.Fh + im.Fo)) return;
    const int v = c.faces[3 * (size_t)im.f_off + t], face = im.f_off + t / 3, corner = t % 3;
    inc_tmp[inc_off[v] + atomicAdd(&cursor[v], 1)] = (face << 2) | corner;
}

// per vertex (all Vtot capacity slots; slots past an image's actual count have empty lists): topo_vertex (k_topo.inc) from the
// temporary list into the tables, with the pair table.  Hand vertices get neighbour lists too but only object vertices are checked.
// A vertex that fails (flag bit 5 of the image that owns it) with more than TOPO_MAXVAL faces has nothing written.
__global__ __launch_bounds__(TOPO_TPB) void k_topo_finish_b(const int32_t* faces, int Vtot, int Fkey, const uint8_t* obj_flag,
                                                            const int32_t* inc_off, const int32_t* inc_tmp, int32_t* inc_fc,
                                                            int32_t* nbr_idx, unsigned long long* pair_v, const foho_image* img, int B,
                                                            int32_t* flags, int32_t* cnt, int32_t* cursor) {
    __shared__ int s_e[TOPO_LDS_LIST], s_d[TOPO_LDS_LIST], s_p[TOPO_LDS_LIST];
    const int v = blockIdx.x * TOPO_TPB + threadIdx.x, t = threadIdx.x * TOPO_LDS_STRIDE;
    if (v >= Vtot) return;
    const int e0 = inc_off[v], n = inc_off[v + 1] - e0;
    cnt[v] = 0;  // counters go back clean for the next iteration
    cursor[v] = 0;
    if (n <= 0) return;
    const int st = topo_vertex<true, true>(faces, inc_tmp, e0, n, Fkey, obj_flag[v] != 0, inc_fc, nbr_idx, pair_v, s_e + t, s_d + t, s_p + t);
    if (st)
        for (int b = 0; b < B; b++)
            if (v >= img[b].v_off && v < img[b].v_off + img[b].Vh + img[b].Vo) atomicOr(&flags[b], 32);
}

// counters over Vtot + 1 items (the scan of the extra zero is the closing offset); the tail is the temporary incidence list
static TopoWs carve_object(void* ws, int32_t Vtot, int32_t Ftot) { return carve_topo(ws, (size_t)Vtot + 1, (size_t)Ftot * 3 * 4); }

extern "C" size_t foho_object_workspace_bytes(int32_t Vtot, int32_t Ftot) {
    return (Vtot < 1 || Ftot < 1) ? 0 : carve_object(nullptr, Vtot, Ftot).total;
}

// The workspace must be zero-filled before its FIRST use; the kernels hand the counters back zeroed.
extern "C" int foho_object_update(const foho_step_desc* desc, const int32_t* counts, const int64_t* obj_faces,
                                  int32_t faces_cap, const uint8_t* obj_flag, void* workspace, size_t workspace_bytes,
                                  void* stream_) {
    if (!desc || !counts || !obj_faces || !obj_flag || faces_cap < 0) {
        foho_set_error("foho_object_update: null argument");
        return FOHO_ERR_BAD_ARG;
    }
    const foho_dims& d = desc->dims;
    if (d.B < 1 || d.Vtot < 1 || d.Ftot < 1 || d.Ftot >= (1 << 28) || d.Fmax < 1 || faces_cap > d.Fo_max) {
        foho_set_error("foho_object_update: bad dims (Vo_max / Fo_max are the per-image object capacities)");
        return FOHO_ERR_BAD_ARG;
    }
    if (!pair_limits_ok(d)) {  // the pair table k_topo_finish_b writes (pack_pair)
        foho_set_error("foho_object_update: more than 4194304 vertex slots per batch or 524287 per image is not supported (pair table)");
        return FOHO_ERR_BAD_ARG;
    }
    const WS w = make_ws(d);
    if (!desc->workspace || desc->workspace_bytes < w.total || !workspace ||
        workspace_bytes < foho_object_workspace_bytes(d.Vtot, d.Ftot)) {
        foho_set_error("foho_object_update: workspace too small (foho_step_workspace_bytes / foho_object_workspace_bytes)");
        return FOHO_ERR_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    Ctx c = make_ctx(*desc, w);
    const TopoWs t = carve_object(workspace, d.Vtot, d.Ftot);
    int32_t* inc_tmp = (int32_t*)t.tail;
    const int fgrid = cdiv(3 * d.Fmax, 256);
    hipLaunchKernelGGL(k_object_adopt, dim3(std::max(1, std::min(fgrid, 128)), d.B), dim3(256), 0, stream, c,
                       const_cast<foho_image*>(desc->images), const_cast<int32_t*>(desc->faces), counts, obj_faces, d.Vo_max, faces_cap, t.cnt);
    CHECK_LAUNCH("k_object_adopt");
    if (const int rc = topo_scan(t, (size_t)d.Vtot + 1, const_cast<int32_t*>(desc->inc_off), stream)) return rc;
    BboxCfg bc;
    bc.nbh = cdiv(d.Vh_max > 0 ? d.Vh_max : 1, 256);
    bc.nbo = cdiv(d.Vo_max > 0 ? d.Vo_max : 1, 256);
    hipLaunchKernelGGL(k_object_fill, dim3(fgrid + bc.nbh + bc.nbo, d.B), dim3(256), 0, stream, c, bc, fgrid, desc->inc_off, t.cursor, inc_tmp);
    CHECK_LAUNCH("k_object_fill");
    hipLaunchKernelGGL(k_topo_finish_b, dim3(cdiv(d.Vtot, TOPO_TPB)), dim3(TOPO_TPB), 0, stream, desc->faces, d.Vtot, d.Ftot, obj_flag, desc->inc_off,
                       inc_tmp, const_cast<int32_t*>(desc->inc_fc), const_cast<int32_t*>(desc->nbr_idx), c.pair_v, desc->images, d.B,
                       desc->flags, t.cnt, t.cursor);
    CHECK_LAUNCH("k_topo_finish_b");
    return FOHO_OK;
}
