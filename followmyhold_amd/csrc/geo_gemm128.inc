// geo_gemm128.inc -- the GEMM of foho_geo.hip on 128 x 128 x 64 tiles: what one wave owns of such a tile (Tile128) and the three kernels that
// differ only in how the LDS ring is filled and waited for, and by which waves.  Included by foho_geo.hip inside namespace geo, behind
// gemm_epilogue64, lds_addr and GEO_DSR.

// A wave's share of a workgroup's 128 x 128 output tile: four waves x (64 x 64).  STAGES: depth of the LDS ring of K tiles.
template <int STAGES>
struct Tile128 {
    typedef uint4 Ring[STAGES][2][GM * GK * 2 / 16];  // [stage][A | W][128 rows x 8 chunks]: 32 KB per stage
    int m0, n0;                    // first row / column of the tile
    int w, wr, wc;                 // the wave (0-3) and its 64 x 64 part of the tile
    const h16 *asrc[4], *wsrc[4];  // this lane's 16 bytes of the wave's four pieces of A and W at K tile 0
    unsigned aa[4], aw[4];         // LDS byte addresses of this lane's A / W fragments in stage 0, by k step
    f32x16 acc[2][2];              // [n tile][m tile]: D rows = n, D columns = m (the lane holds 4 consecutive n for one m)

    // false: the tile lies beyond the last row (the grid is padded to whole groups of eight row panels) -- the workgroup leaves
    __device__ __forceinline__ bool setup(const Ring& lds, const h16* __restrict__ A, int lda, const h16* __restrict__ Wt, int ldw, int M, int N, int lane,
                                          int wave) {
        const int hi = lane >> 5, l31 = lane & 31;
        w = wave;
        // XCD-aware tile order: the blocks of one XCD (L mod 8) sweep N inside one row panel of A, eight panels (one per XCD) at a time
        const int ntn = N / GN, ntm = (M + GM - 1) / GM;
        const int L = blockIdx.x, xcd = L & 7, j = L >> 3;
        const int mp = (j / ntn) * 8 + xcd, nt = j % ntn;
        if (mp >= ntm) return false;
        m0 = mp * GM, n0 = nt * GN;
        wr = w >> 1, wc = w & 1;

        // Staging by LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 B = 8 rows of a tile per instruction, destination lane-linear,
        // so the XOR swizzle sits on the SOURCE address): no VGPR -> LDS store pass -- register staging had this kernel bound by
        // the LDS (ds_write_b128 costs 13 cycles per wave-instruction: 832 of them + 512 of fragment reads per K-tile and CU
        // against 1024 cycles of MFMA).  A wave moves pieces w*4 .. w*4+3 of both operands per K-tile.
        const int srow = lane >> 3, sslot = lane & 7;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = (w * 4 + p) * 8 + srow;
            const int c = sslot ^ swz(row);
            asrc[p] = A + (size_t)min(m0 + row, M - 1) * lda + c * 8;
            wsrc[p] = Wt + (size_t)(n0 + row) * ldw + c * 8;
        }

#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;

        // fragment byte addresses inside stage 0: row r, chunk c -> r * 128 + (c ^ swz(r)) * 16; the second tile of a wave
        // (rows + 32, same swizzle) is an immediate offset of 4096, the W operand one of 16384
        const int ra = wr * 64 + l31, rw = wc * 64 + l31;
        const unsigned base = lds_addr(&lds[0][0][0]);
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            aa[kk] = base + ra * 128 + (((2 * kk + hi) ^ swz(ra)) << 4);
            aw[kk] = base + rw * 128 + (((2 * kk + hi) ^ swz(rw)) << 4);
        }
        return true;
    }

    // issues this wave's eight pieces of K tile t into stage t mod STAGES
    __device__ __forceinline__ void fill(Ring& lds, int t) const {
        const int sb = t & (STAGES - 1), k0 = t * GK;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            glds16(asrc[p] + k0, &lds[sb][0][(w * 4 + p) * 64]);
            glds16(wsrc[p] + k0, &lds[sb][1][(w * 4 + p) * 64]);
        }
    }

    // acc += K tile t (in its stage of the ring, published to this wave by the caller's barrier).  The fragment reads are INLINE ASM:
    // hipcc cannot tell the DMA's destination stage from the one being read and waits vmcnt(0) in front of every compiler-visible
    // ds_read, which serialises the prefetch with the MFMAs (measured: the first version of k_geo_gemm); reads it cannot see get no such
    // wait, and this code counts lgkmcnt itself.  STAMPS: the P8_STAMP hooks 4 and 5 of a -DP8_STAMPS build (k_geo_gemm_d4; ts: its stamps).
    template <bool STAMPS = false>
    __device__ __forceinline__ void multiply(int t, unsigned long long* ts = nullptr) {
        asm volatile("" ::: "memory");
        const unsigned bo = (unsigned)(t & (STAGES - 1)) << 15;  // 32 KB per stage
        half8 fa[2][2], fw[2][2];  // [parity of kk][tile]: the fragments of step kk + 1 are requested before step kk's MFMAs issue
        {
            const unsigned pa = aa[0] + bo, pw = aw[0] + bo;
            GEO_DSR(fa[0][0], pa, 0);
            GEO_DSR(fa[0][1], pa, 4096);
            GEO_DSR(fw[0][0], pw, 16384);
            GEO_DSR(fw[0][1], pw, 16384 + 4096);
        }
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            if (kk < 3) {
                const unsigned pa = aa[kk + 1] + bo, pw = aw[kk + 1] + bo;
                GEO_DSR(fa[(kk + 1) & 1][0], pa, 0);
                GEO_DSR(fa[(kk + 1) & 1][1], pa, 4096);
                GEO_DSR(fw[(kk + 1) & 1][0], pw, 16384);
                GEO_DSR(fw[(kk + 1) & 1][1], pw, 16384 + 4096);
                // LDS returns in order: at most the four reads just issued may still be out
                asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(fa[kk & 1][0]), "+v"(fa[kk & 1][1]), "+v"(fw[kk & 1][0]), "+v"(fw[kk & 1][1]));
                if (STAMPS && kk == 0) P8_STAMP(4);
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[kk & 1][0]), "+v"(fa[kk & 1][1]), "+v"(fw[kk & 1][0]), "+v"(fw[kk & 1][1]));
            }
#pragma unroll
            for (int jn = 0; jn < 2; jn++)
#pragma unroll
                for (int i = 0; i < 2; i++)
                    acc[jn][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[kk & 1][jn], fa[kk & 1][i], acc[jn][i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (STAMPS && kk == 1) P8_STAMP(5);
        }
    }

    // the wave's 64 x 64 part through gemm_epilogue64; every wave is done with the ring: it is the waves' transpose images now
    template <int EP>
    __device__ __forceinline__ void epilogue(Ring& lds, const float* __restrict__ bias, const h16* __restrict__ R, int ldr, h16* __restrict__ C, int ldc,
                                             h16* __restrict__ C2, int ldc2, int M, float scale, int lane, const EpiAux& aux) const {
        h16* img = reinterpret_cast<h16*>(&lds[0][0][0]) + w * (64 * CPAD);
        EpiCols pc;
        EpiRows pr;
        epi_cols<EP>(pc, bias, ldr, ldc2, n0 + wc * 64, lane);
        epi_rows<EP>(pr, R, ldr, M, m0 + wr * 64, n0 + wc * 64, lane);
        gemm_epilogue64<EP>(acc[0][0], acc[0][1], acc[1][0], acc[1][1], img, pc, pr, R, C, ldc, C2, ldc2, M, scale, m0 + wr * 64, n0 + wc * 64, lane, bias, ldr, aux);
    }
};

// Four-deep ring: before the barrier that publishes K tile t, a wave waits until its own pieces of that tile have landed -- at most the
// pieces of the newer tiles in flight (two tiles of 8 pieces in the steady state) remain outstanding.
__device__ __forceinline__ void ring4_wait(int t, int nk) {
    if (t + 2 < nk) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (t + 1 < nk) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------------------
// Two stages: tile t + 1 is in flight while tile t is multiplied; vmcnt(0) + __syncthreads() per K tile.
// ------------------------------------------------------------------------------------------------
template <int EP>
__global__ __launch_bounds__(256, 2) void k_geo_gemm(const h16* __restrict__ A, int lda, const h16* __restrict__ Wt, int ldw,
                                                     const float* __restrict__ bias, const h16* __restrict__ R, int ldr,
                                                     h16* __restrict__ C, int ldc, int M, int N, int K, float scale, h16* __restrict__ C2,
                                                     int ldc2, const int* __restrict__ Mdev, EpiAux aux = EpiAux{}) {
    __shared__ Tile128<2>::Ring lds;  // 64 KB
    if (Mdev) M = min(M, *Mdev);   // device-resident row count (foho_geo_decode_bwd_rows): tiles beyond it leave at once
    const int tid = threadIdx.x, lane = tid & 63;
    Tile128<2> T;
    if (!T.setup(lds, A, lda, Wt, ldw, M, N, lane, tid >> 6)) return;
    const int nk = K / GK;
    T.fill(lds, 0);
    for (int t = 0; t < nk; t++) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // tile t has landed for every wave, and everybody is done reading the other buffer
        if (t + 1 < nk) T.fill(lds, t + 1);
        T.multiply(t);
    }
    __syncthreads();  // every wave is done with the staging buffers: they become the epilogue's transpose image
    T.template epilogue<EP>(lds, bias, R, ldr, C, ldc, C2, ldc2, M, scale, lane, aux);
}

// ------------------------------------------------------------------------------------------------
// The 128 x 128 x 64 GEMM with a FOUR-deep LDS ring (round 6), for launches that put at most one workgroup on a CU -- the N = 1024
// products of the ShapeVAE transformer at M = 3072 (192 tiles on 256 CUs: c_proj, fc2 and the three transposed-weight GEMMs of the
// backward).  k_geo_gemm issues a tile's eight LDS-DMA pieces per wave in one block in front of the tile's matrix instructions; a wave
// is held ~80 cycles per piece, and with ONE wave per SIMD (one workgroup per CU) nothing else feeds the matrix pipe meanwhile:
// 0.65 us per K tile against 0.21 us of matrix work (0.93 us inside the transformer chain: 59 us for K = 4096).  A deeper ring ALONE
// changed nothing (measured: the latency was never the limit).  Here tile t + 3 is issued while tile t is multiplied (4 x 32 KB of
// LDS) and a wave waits for
// its OWN oldest tile with a counted s_waitcnt vmcnt(16) (two newer tiles of 8 pieces stay in flight) before the barrier that
// publishes the tile to the other waves.  Same fragments, same epilogue as k_geo_gemm.
// ------------------------------------------------------------------------------------------------
template <int EP>
__global__ __launch_bounds__(256, 1) void k_geo_gemm_d4(const h16* __restrict__ A, int lda, const h16* __restrict__ Wt, int ldw,
                                                        const float* __restrict__ bias, const h16* __restrict__ R, int ldr,
                                                        h16* __restrict__ C, int ldc, int M, int N, int K, float scale, h16* __restrict__ C2,
                                                        int ldc2, const int* __restrict__ Mdev, EpiAux aux = EpiAux{}) {
    __shared__ Tile128<4>::Ring lds;  // 128 KB
    if (Mdev) M = min(M, *Mdev);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    Tile128<4> T;
    if (!T.setup(lds, A, lda, Wt, ldw, M, N, lane, w)) return;
    const int nk = K / GK;
    for (int t = 0; t < 3 && t < nk; t++) T.fill(lds, t);
    P8_STAMP_DECL;   // (development builds -DP8_STAMPS: per-wave sums of a K tile's segments, foho_geo_stamps.h; empty otherwise)
    for (int t = 0; t < nk; t++) {
        ring4_wait(t, nk);
        P8_STAMP(1);
        // RAW barrier: __syncthreads() fences with s_waitcnt vmcnt(0) -- an LDS-DMA in flight is a pending LDS write -- and would drain the
        // ring at every tile (the first build of this kernel did: no faster than two stages).  This wave's own reads of stage (t - 1) & 3
        // completed with the lgkmcnt(0) of the previous tile's last k step.
        __builtin_amdgcn_s_barrier();  // tile t has landed for every wave, and everybody is done reading stage (t - 1) & 3 -- where tile t + 3 goes
        P8_STAMP(2);
        if (t + 3 < nk) T.fill(lds, t + 3);   // (in ONE block: two pieces behind each k step's matrix instructions measured 55.6 against 41.8 us at K = 4096)
        P8_STAMP(3);
#ifdef D4_FILL_ONLY   // (development build: the ring's fill alone -- no fragment reads, no matrix instructions; results are garbage)
        continue;
#endif
        T.template multiply<true>(t, P8_STAMP_TS);
        P8_STAMP(6);
        P8_ACC();
    }
    P8_STAMP_DUMP(w, nk);
    __syncthreads();  // every wave is done with the ring: it becomes the epilogue's transpose image
    T.template epilogue<EP>(lds, bias, R, ldr, C, ldc, C2, ldc2, M, scale, lane, aux);
}

// ------------------------------------------------------------------------------------------------
// k_geo_gemm_d4 with the FILL and the MATRIX work on different waves (round 6): a CU fills its LDS at ~86 GB/s (382 ns per 32 KB K tile)
// and a wave that issues LDS-DMA issues nothing else, so at one wave per SIMD fill time and matrix time add (0.68 us per K tile,
// NOTEBOOK round 6).  Eight waves: waves 4-7 only fill the four-deep ring, waves 0-3 only read fragments and multiply; one raw barrier
// per K tile hands tile t over and frees stage (t - 1) & 3.  The consumers run the epilogue.
// ------------------------------------------------------------------------------------------------
template <int EP>
__global__ __launch_bounds__(512, 1) void k_geo_gemm_pc(const h16* __restrict__ A, int lda, const h16* __restrict__ Wt, int ldw,
                                                        const float* __restrict__ bias, const h16* __restrict__ R, int ldr,
                                                        h16* __restrict__ C, int ldc, int M, int N, int K, float scale, h16* __restrict__ C2,
                                                        int ldc2, const int* __restrict__ Mdev, EpiAux aux = EpiAux{}) {
    __shared__ Tile128<4>::Ring lds;  // 128 KB
    if (Mdev) M = min(M, *Mdev);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool producer = wv >= 4;   // waves 4-7 only FILL the ring (each the eight pieces wave wv - 4 would), waves 0-3 only multiply
    Tile128<4> T;
    if (!T.setup(lds, A, lda, Wt, ldw, M, N, lane, wv & 3)) return;
    const int nk = K / GK;
    if (producer) {
        for (int t = 0; t < 3 && t < nk; t++) T.fill(lds, t);
        for (int t = 0; t < nk; t++) {
            ring4_wait(t, nk);
            __builtin_amdgcn_s_barrier();   // tile t has landed (every producer waited for its pieces); the consumers are done with tile t - 1
            if (t + 3 < nk) T.fill(lds, t + 3);
        }
        __syncthreads();
        return;
    }
    for (int t = 0; t < nk; t++) {
        __builtin_amdgcn_s_barrier();
        T.multiply(t);
    }
    __syncthreads();  // every wave is done with the ring: it becomes the epilogue's transpose image
    T.template epilogue<EP>(lds, bias, R, ldr, C, ldc, C2, ldc2, M, scale, lane, aux);
}
