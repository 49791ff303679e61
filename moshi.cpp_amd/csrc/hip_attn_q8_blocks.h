// hip_attn_q8_blocks.h - slot prefill over Q8_0 K / V rings (moshi_hot_config::kv_q8 = 3): the attention blocks of one layer of one pass,
// job j = T_j new rows on its own column of the [D, C, H, B] rings, as a PAIR of launches - attn_blocks_q8_write_kernel<D>, then
// attn_blocks_q8_attend_kernel<D>; launcher k_attn_blocks_q8. Included by hip_kernels_fused.hip behind hip_attn_q8.h, whose shapes, tile copy routine and
// row quantiser it uses. The contract is that header's (ggml's arithmetic for set_rows into Q8_0, vec_dot_q8_0_q8_0, soft_max, get_rows, F32 x F32), with
// ONE departure: float(v) * p is kept exact in double instead of being rounded to float before the double sum (what f32_matrix does for F32 weights).
// No workgroup waits for another, no workspace, no scratch: the launch boundary is the write-then-attend order of a [dim, T] pass.
//
// WRITE LAUNCH, grid (H, jobs). A workgroup rotates the job's T k-rows as apply_rope does and quantises its k- and v-rows (attn_q8_rope_quant: D / 4
// lanes a row, 1024 / D rows a pass), leaves them in LDS in ggml's row format and stores them to their ring slots packed (8 bytes at D = 128, 4 at 64).
//
// ATTEND LAUNCH, grid (ceil(T_max / 16), H, jobs), 256 threads = 4 waves. A workgroup owns 16 query rows of one (job, head); a tile past the job's end
// leaves at once.
//   head      the 16 q rows rotated and quantised into LDS: 16 x D int8 (row pitch D + 8: the sixteen rows a matrix operand reads fall into different
//             banks) and 16 x D / 32 float scales; rows past T_j are zeros with scale 0. The mask block's 16 rows are scanned for the tile's live end
//             n_end, the largest un-masked slot of any of its rows; nothing past it is read.
//   ring walk the K column of the head in raw 128-slot byte tiles (attn_q8_request / attn_q8_store: no byte outside the range is touched) through two
//             LDS buffers, tile t + 1 requested before tile t is consumed. A tile's quants are re-packed ONCE into an aligned image - slot s at
//             s x (D + 8), its blocks' F16 scales beside it - because the matrix operand wants 8 consecutive int8 per lane and a ring block starts on any
//             even byte.
//   scores    wave w takes the 16-slot groups 2 w and 2 w + 1 of the tile. Per block j one v_mfma_i32_16x16x32_i8: lane l = (r = l & 15, g = l >> 4)
//             supplies A = bytes 32 j + 8 g .. + 7 of q row r and B = the same bytes of slot r of the group, and receives the exact integer dots of rows
//             4 g + q, q = 0 .. 3, with slot r. term = float(dot) * (h2f(d_k) * d_q), the block terms added in float in block order, then * scale, + mask:
//             vec_dot_q8_0_q8_0 and soft_max's input, bit for bit. attn_q8_tile_scores is the one instruction sequence of all three walks.
//   3 walks   16 x 4096 float scores do not fit beside the tiles, so they are recomputed, not stored: walk 1 (K) the row maxima; walk 2 (K)
//             e = expf(s - max) summed in double per row - a lane's slots in ascending order, the sixteen lanes of a row by DPP, the waves in index
//             order - and inv = float(1 / sum); walk 3 (K and V tiles side by side in the two buffers) p = e * inv into a 16 x 128 float tile, then
//   P x V     v_mfma_f64_16x16x4_f64 with mm_op_f64_f32's lane map: A = double(p[row r][slot 4 s + g]), B = double(h2f(d_v) * q_v) of slot 4 s + g,
//             dim 16 dt + r (the product of an F16 and an int8 is exact in float), D[row g + 4 q][dim 16 dt + r] in register q. The D / 16 dim tiles
//             are dealt to the waves (two each at D = 128, one at 64); each accumulates over ALL slots in ascending order; one rounding to float.
//   A slot past a row's own live end carries p = 0 through the mask; a row with no live slot writes zeros. A row's bits depend on its own job alone.
//   Everything behind the head is attn_q8b_walks, a function: the rows form (hip_attn_q8_rows.h) runs the same walks with an overlay of new rows.
#pragma once

#define ATTN_Q8B_ROWS 16   // query rows of a workgroup: the M of both matrix instructions
#define ATTN_Q8B_PP 132    // floats between two rows of the probability tile (128 + 4: sixteen rows, sixteen banks)

template <int D> struct attn_q8b_shape {
    typedef attn_q8_shape<D> S;
    static constexpr int PITCH = D + 8;                                    // bytes between two rows of the q image and between two slots of the K image
    static constexpr int O_KIMG = 2 * S::BUF_Q8_BYTES, O_KD = O_KIMG + ATTN_Q8_TILE * PITCH, O_P = O_KD + ATTN_Q8_TILE * S::NBLK * 2;
    static constexpr int O_QQ = O_P + ATTN_Q8B_ROWS * ATTN_Q8B_PP * 4, O_QD = O_QQ + ATTN_Q8B_ROWS * PITCH, O_REDD = O_QD + ATTN_Q8B_ROWS * S::NBLK * 4;
    static constexpr int O_REDF = O_REDD + 4 * ATTN_Q8B_ROWS * 8, O_STAT = O_REDF + 4 * ATTN_Q8B_ROWS * 4, O_REDI = O_STAT + 2 * ATTN_Q8B_ROWS * 4;
    static constexpr int SMEM = O_REDI + 16;
    static_assert(SMEM <= 64 * 1024 && O_KIMG % 16 == 0 && O_REDD % 8 == 0 && PITCH % 8 == 0, "LDS of the attend launch: under the 64 KB every launch may have");
};

// what the three walks work in (LDS): the two raw tile buffers, the aligned K image and its scales, the probability tile, the quantised query rows and
// their scales, the reduction rows, the row maxima and reciprocal sums
struct attn_q8b_lds { char * buf0, * buf1, * kimg; uint16_t * kd; float * P; const char * qq; const float * qd; double * redd; float * redf, * rmax, * rinv; };
// the rows form's overlay (hip_attn_q8_rows.h): n <= 16 new rows that stand in LDS and not yet in the ring - K as an aligned image (row j at kimg + j * PITCH,
// scales kd[j * NBLK + block]), V in ggml's row format, slot[j] the ring slot row j will take (-1: none; 16 entries)
struct attn_q8b_overlay { const char * kimg = nullptr; const uint16_t * kd = nullptr; const char * vrows = nullptr; const int * slot = nullptr; int n = 0; };
template <int D, bool OV>
__device__ __forceinline__ void attn_q8b_walks(const attn_q8b_lds & m, const attn_q8b_overlay & ov, const char * kring, const char * vring, const float * (&mrow)[4],
                                               int nrows, int n_end, int C, float scale, float * out, int64_t out_ts);

// ---- write launch ------------------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(ATTN_Q8_THREADS) attn_blocks_q8_write_kernel(attn_blocks_args ba) {
    typedef attn_q8_shape<D> S;
    constexpr int ROWB = S::ROWB, half = D / 2, LPR = D / 4, RPP = ATTN_Q8_THREADS / LPR, PIECE = D == 128 ? 8 : 4, NPC = ROWB / PIECE;
    __shared__ __attribute__((aligned(16))) char rows[RPP * S::ROW_Q8_BUF];
    const attn_block_job & jb = ba.job[blockIdx.y];
    const attn_args & a = ba.a;
    const int tid = threadIdx.x, h = blockIdx.x, T = jb.T;
    const int ur = tid / LPR, ln = tid % LPR, j0 = ln * 4;
    for (int u0 = 0; u0 < 2 * T; u0 += RPP) {                              // unit u: k row u (u < T), v row u - T
        const int u = u0 + ur, kv = u >= T, t = u - kv * T;
        float in0[4], in1[4], rc[4], rs[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { in0[i] = 0.f; in1[i] = 0.f; rc[i] = 1.f; rs[i] = 0.f; }
        const bool rotate = !kv && jb.rot;
        if (u < 2 * T) {
            const float * src = kv ? jb.v + (int64_t) t * a.v_ts + (int64_t) h * a.v_hs : jb.k + (int64_t) t * a.k_ts + (int64_t) h * a.k_hs;
            if (rotate) {
                const float * rot = jb.rot + (int64_t) t * D;
                const int p0 = j0 < half ? j0 : j0 - half;
#pragma unroll
                for (int i = 0; i < 4; i++) { in0[i] = src[2 * (p0 + i)]; in1[i] = src[2 * (p0 + i) + 1]; rc[i] = rot[p0 + i]; rs[i] = rot[half + p0 + i]; }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) in0[i] = src[j0 + i];
            }
        }
        uint16_t dh;
        const uint32_t packed = attn_q8_rope_quant(in0, in1, rc, rs, rotate, j0 >= half, dh);
        char * row = rows + ur * S::ROW_Q8_BUF + (ln >> 3) * 34;            // block ln / 8: d, then the quants 2 bytes in
        uint16_t * qs = (uint16_t *) (row + 2 + (ln & 7) * 4);
        qs[0] = (uint16_t) (packed & 0xffff); qs[1] = (uint16_t) (packed >> 16);
        if ((ln & 7) == 0) *(uint16_t *) row = dh;
        __syncthreads();
        for (int p = tid; p < RPP * NPC; p += ATTN_Q8_THREADS) {           // the rows of this pass to their ring slots, packed
            const int pr = p / NPC, pc = p % NPC, pu = u0 + pr;
            if (pu >= 2 * T) continue;
            const int pkv = pu >= T, slot = jb.index[pu - pkv * T];
            if (slot < 0 || slot >= a.C) continue;
            char * dst = (pkv ? jb.vcache + (int64_t) h * a.v_nb2 + (int64_t) slot * a.v_nb1 : jb.kcache + (int64_t) h * a.k_nb2 + (int64_t) slot * a.k_nb1) + pc * PIECE;
            const char * from = rows + pr * S::ROW_Q8_BUF + pc * PIECE;
            if (D == 128) *(uint2 *) dst = *(const uint2 *) from; else *(uint32_t *) dst = *(const uint32_t *) from;
        }
        __syncthreads();
    }
}

// ---- attend launch -----------------------------------------------------------------------------------------------------------------------------------
// the quants and scales of the raw tile in `buf` (its first slot off0 bytes in) into the aligned image: slot s at kimg + s * PITCH, scale (s, j) at kd[s * NBLK + j]
template <int D> __device__ __forceinline__ void attn_q8b_repack(const char * buf, int off0, char * kimg, uint16_t * kd) {
    typedef attn_q8_shape<D> S;
    constexpr int NBLK = S::NBLK, PITCH = attn_q8b_shape<D>::PITCH;
#pragma unroll
    for (int pass = 0; pass < ATTN_Q8_TILE * NBLK / ATTN_Q8_THREADS; pass++) {
        const int u = pass * ATTN_Q8_THREADS + threadIdx.x, s = u / NBLK, j = u % NBLK;
        const int A = off0 + s * S::ROWB + j * 34;                          // the block: even, not always a dword boundary
        const uint32_t * w = (const uint32_t *) (buf + (A & ~3));
        const bool odd = (A & 2) != 0;
        uint32_t wv[9];
#pragma unroll
        for (int i = 0; i < 9; i++) wv[i] = w[i];
        kd[s * NBLK + j] = (uint16_t) (odd ? wv[0] >> 16 : wv[0] & 0xffff);
        uint32_t * o = (uint32_t *) (kimg + s * PITCH + j * 32);
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = odd ? wv[i + 1] : __builtin_amdgcn_alignbyte(wv[i + 1], wv[i], 2);
    }
}

// the block terms of rows 4 g + q, q = 0 .. 3, of the workgroup against slot sl = 16 grp + r of the K image, added in float in block order: sumf[q]
template <int D> __device__ __forceinline__ void attn_q8_tile_dots(const char * qq, const float * qd, const char * kimg, const uint16_t * kd, int grp, float (&sumf)[4]) {
    constexpr int NBLK = attn_q8_shape<D>::NBLK, PITCH = attn_q8b_shape<D>::PITCH;
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4, sl = 16 * grp + r;
#pragma unroll
    for (int q = 0; q < 4; q++) sumf[q] = 0.f;
#pragma unroll
    for (int j = 0; j < NBLK; j++) {
        const long aq = *(const long *) (qq + r * PITCH + 32 * j + 8 * g), bk = *(const long *) (kimg + sl * PITCH + 32 * j + 8 * g);
        const i32x4_t z = { 0, 0, 0, 0 };
        const i32x4_t dot = __builtin_amdgcn_mfma_i32_16x16x32_i8(aq, bk, z, 0, 0, 0);
        const float dk = h2f(kd[sl * NBLK + j]);
#pragma unroll
        for (int q = 0; q < 4; q++) sumf[q] += (float) dot[q] * (dk * qd[(4 * g + q) * NBLK + j]);
    }
}
// soft_max's input from the summed block terms and the mask value m of the (row, slot) pair (-inf: the pair is closed)
__device__ __forceinline__ float attn_q8_masked_score(float sumf, float scale, float m) {
    float sv = -INFINITY;
    if (m > -INFINITY) { sv = sumf * scale; sv = sv + m; }
    return sv;
}
// the scores of rows 4 g + q, q = 0 .. 3, of the workgroup against slot c = c0 + 16 grp + r of the tile in the K image: sv[q], masked and scaled
// (mrow[q]: the mask row of row 4 g + q, NULL for a row past the job's end; a slot at or past C is masked)
template <int D> __device__ __forceinline__ void attn_q8_tile_scores(const char * qq, const float * qd, const char * kimg, const uint16_t * kd, const float * (&mrow)[4],
                                                                     int c0, int grp, int C, float scale, float (&sv)[4]) {
    const int c = c0 + 16 * grp + (threadIdx.x & 15);
    float sumf[4];
    attn_q8_tile_dots<D>(qq, qd, kimg, kd, grp, sumf);
#pragma unroll
    for (int q = 0; q < 4; q++) sv[q] = attn_q8_masked_score(sumf[q], scale, mrow[q] && c < C ? mrow[q][c] : -INFINITY);
}

template <int D>
__global__ void __launch_bounds__(ATTN_Q8_THREADS) attn_blocks_q8_attend_kernel(attn_blocks_args ba) {
    typedef attn_q8_shape<D> S;
    typedef attn_q8b_shape<D> L;
    constexpr int NBLK = S::NBLK, half = D / 2, PITCH = L::PITCH, R = ATTN_Q8B_ROWS, LPR = D / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const attn_block_job & jb = ba.job[blockIdx.z];
    const int r0 = (int) blockIdx.x * R;
    if (r0 >= jb.T) return;                                                 // (the grid is as wide as the longest job)
    const attn_args & a = ba.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int h = blockIdx.y, C = a.C, nrows = jb.T - r0 < R ? jb.T - r0 : R;

    char * const buf0 = smem, * const buf1 = smem + S::BUF_Q8_BYTES;          // the two tile buffers
    char * kimg = smem + L::O_KIMG; uint16_t * kd = (uint16_t *) (smem + L::O_KD);
    float * P = (float *) (smem + L::O_P);
    char * qq = smem + L::O_QQ; float * qd = (float *) (smem + L::O_QD);
    double * redd = (double *) (smem + L::O_REDD); float * redf = (float *) (smem + L::O_REDF);
    float * rmax = (float *) (smem + L::O_STAT), * rinv = rmax + R;
    int * redi = (int *) (smem + L::O_REDI);

    const char * kring = jb.kcache + (int64_t) h * a.k_nb2, * vring = jb.vcache + (int64_t) h * a.v_nb2;
    float * out = jb.out + (int64_t) r0 * a.out_ts + (int64_t) h * D;

    // ---- head: the q rows, rotated and quantised; the live end of the tile's rows ----------------------------------------------------------------
#pragma unroll
    for (int pass = 0; pass < R * LPR / ATTN_Q8_THREADS; pass++) {
        const int u = pass * ATTN_Q8_THREADS + tid, row = u / LPR, ln = u % LPR, j0 = ln * 4;
        float in0[4], in1[4], rc[4], rs[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { in0[i] = 0.f; in1[i] = 0.f; rc[i] = 1.f; rs[i] = 0.f; }
        if (row < nrows) {
            const float * src = jb.q + (int64_t) (r0 + row) * a.q_ts + (int64_t) h * a.q_hs;
            if (jb.rot) {
                const float * rot = jb.rot + (int64_t) (r0 + row) * D;
                const int p0 = j0 < half ? j0 : j0 - half;
#pragma unroll
                for (int i = 0; i < 4; i++) { in0[i] = src[2 * (p0 + i)]; in1[i] = src[2 * (p0 + i) + 1]; rc[i] = rot[p0 + i]; rs[i] = rot[half + p0 + i]; }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) in0[i] = src[j0 + i];
            }
        }
        uint16_t dh;
        const uint32_t packed = attn_q8_rope_quant(in0, in1, rc, rs, jb.rot != nullptr, j0 >= half, dh);
        *(uint32_t *) (qq + row * PITCH + j0) = packed;
        if ((ln & 7) == 0) qd[row * NBLK + (ln >> 3)] = h2f(dh);
    }
    {
        int last = -1;
        const int row = tid >> 4;
        if (row < nrows) {
            const float * mr = jb.mask + (int64_t) (r0 + row) * C;
            for (int c = tid & 15; c < C; c += 16) if (mr[c] > -INFINITY) last = c;   // (ascending c: the last hit is the largest)
        }
        last = wave_allmax_i32(last);
        if (lane == 0) redi[wave] = last;
    }
    __syncthreads();
    const int n_end = max(max(redi[0], redi[1]), max(redi[2], redi[3])) + 1;
    if (n_end <= 0) {   // no row of the tile sees a slot: zeros
        for (int i = tid; i < nrows * D; i += ATTN_Q8_THREADS) out[(int64_t) (i / D) * a.out_ts + i % D] = 0.f;
        return;
    }
    const float * mrow[4];
#pragma unroll
    for (int q = 0; q < 4; q++) mrow[q] = 4 * g + q < nrows ? jb.mask + (int64_t) (r0 + 4 * g + q) * C : nullptr;
    const attn_q8b_lds m = { buf0, buf1, kimg, kd, P, qq, qd, redd, redf, rmax, rinv };
    attn_q8b_walks<D, false>(m, attn_q8b_overlay(), kring, vring, mrow, nrows, n_end, C, a.scale, out, a.out_ts);
}

// THE THREE WALKS of a workgroup whose 16 query rows stand quantised in LDS (m.qq, m.qd), over slots [0, n_end) of the head's ring column, n_end >= 1:
// row r of the workgroup (r < nrows) under its mask row mrow, its output row at out + r * out_ts. Shared with the rows form (hip_attn_q8_rows.h), which
// instantiates OV: ring slots one of its overlay rows has rewritten are switched off per (row, slot) pair and the overlay is one more 16-slot group
// behind the last tile, through the same score function in all three walks. Without OV this is the attend launch's code, instruction for instruction.
template <int D, bool OV>
__device__ __forceinline__ void attn_q8b_walks(const attn_q8b_lds & m, const attn_q8b_overlay & ov, const char * kring, const char * vring, const float * (&mrow)[4],
                                               int nrows, int n_end, int C, float scale, float * out, int64_t out_ts) {
    typedef attn_q8_shape<D> S;
    constexpr int ROWB = S::ROWB, TILE = ATTN_Q8_TILE, PP = ATTN_Q8B_PP, R = ATTN_Q8B_ROWS, NDT = D / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    char * const buf0 = m.buf0, * const buf1 = m.buf1, * const kimg = m.kimg;
    uint16_t * const kd = m.kd;
    float * const P = m.P, * const redf = m.redf, * const rmax = m.rmax, * const rinv = m.rinv;
    double * const redd = m.redd;
    auto buf_of = [&](int t) { return (t & 1) ? buf1 : buf0; };
    const int koff = (int) ((uintptr_t) kring & 15), voff = (int) ((uintptr_t) vring & 15);   // (a tile is a multiple of 16 bytes: every tile of a ring has its alignment)
    const int NT = (n_end + TILE - 1) / TILE;
    auto tile_end = [&](int t) { const int e = (t + 1) * TILE; return e < n_end ? e : n_end; };
    int ovs[OV ? R : 1];   // OV: the overlay rows' ring slots (-1: none)
    if constexpr (OV) {
#pragma unroll
        for (int j = 0; j < R; j++) ovs[j] = ov.slot[j];
    }
    // a tile's scores (attn_q8_tile_scores); OV: a pair whose ring slot an overlay row j <= row has rewritten is closed
    auto scores = [&](int c0, int grp, float (&sv)[4]) {
        attn_q8_tile_scores<D>(m.qq, m.qd, kimg, kd, mrow, c0, grp, C, scale, sv);
        if constexpr (OV) {
            const int c = c0 + 16 * grp + r;
            int first = R;
#pragma unroll
            for (int j = R - 1; j >= 0; j--) if (ovs[j] == c) first = j;
#pragma unroll
            for (int q = 0; q < 4; q++) if (4 * g + q >= first) sv[q] = -INFINITY;
        }
    };
    // OV: the overlay as a 16-slot group - overlay row r against the workgroup's rows; row i sees it from i = r on until a later overlay row takes its slot
    auto overlay_scores = [&](float (&sv)[4]) {
        const int cj = ov.slot[r];
        int next = R;
#pragma unroll
        for (int j = R - 1; j > 0; j--) if (j > r && ovs[j] == cj) next = j;
        float sumf[4];
        attn_q8_tile_dots<D>(m.qq, m.qd, ov.kimg, ov.kd, 0, sumf);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = 4 * g + q;
            sv[q] = attn_q8_masked_score(sumf[q], scale, cj >= 0 && r <= i && i < next && mrow[q] ? mrow[q][cj] : -INFINITY);
        }
    };
    // P x V over `nslots` slots of V rows in ggml's row format at vrows, their probabilities in P's columns 0 .. nslots - 1
    auto pv_steps = [&](const char * vrows, int nslots, f64x4_t (&acc)[NDT]) {
        const int steps = (nslots + 3) / 4;
        for (int s = 0; s < steps; s++) {
            const int sl = 4 * s + g;
            const double pa = (double) P[r * PP + sl];
            const char * vrow = vrows + sl * ROWB;
#pragma unroll
            for (int i = 0; i < NDT; i++) {
                const int dim = 16 * (wave * NDT + i) + r;
                const char * blk = vrow + (dim >> 5) * 34;
                const float v = sl < nslots ? h2f(*(const uint16_t *) blk) * (float) *(const int8_t *) (blk + 2 + (dim & 31)) : 0.f;   // (exact: 11 x 8 significant bits)
                acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, (double) v, acc[i], 0, 0, 0);
            }
        }
    };

    attn_q8_u32x4 regs[S::NPIECE], vregs[S::NPIECE];   // a tile's pieces between their request and their store to LDS
    uint32_t edge, vedge;

    // ---- walks 1 and 2 over K: the row maxima, then the sums of the exponentials -----------------------------------------------------------------
    float mx[4] = { -INFINITY, -INFINITY, -INFINITY, -INFINITY };
    double ds[4] = { 0, 0, 0, 0 };
    for (int walk = 0; walk < 2; walk++) {
        float rm[4];
#pragma unroll
        for (int q = 0; q < 4; q++) rm[q] = walk ? rmax[4 * g + q] : 0.f;
        attn_q8_request<D>(regs, edge, kring, 0, tile_end(0));
        attn_q8_store<D>(regs, edge, buf0, kring, 0, tile_end(0));
        __syncthreads();
        for (int t = 0; t < NT; t++) {
            if (t + 1 < NT) attn_q8_request<D>(regs, edge, kring, (t + 1) * TILE, tile_end(t + 1));
            attn_q8b_repack<D>(buf_of(t), koff, kimg, kd);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2; i++) {
                float sv[4];
                scores(t * TILE, 2 * wave + i, sv);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (walk == 0) mx[q] = fmaxf(mx[q], sv[q]);
                    else ds[q] += (double) (sv[q] > -INFINITY ? expf(sv[q] - rm[q]) : 0.f);
                }
            }
            if (t + 1 < NT) attn_q8_store<D>(regs, edge, buf_of(t + 1), kring, (t + 1) * TILE, tile_end(t + 1));
            __syncthreads();
        }
        if constexpr (OV) if (wave == 0) {   // the overlay group: wave 0's lanes add it behind their ring slots
            float sv[4];
            overlay_scores(sv);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (walk == 0) mx[q] = fmaxf(mx[q], sv[q]);
                else ds[q] += (double) (sv[q] > -INFINITY ? expf(sv[q] - rm[q]) : 0.f);
            }
        }
        // a row's value over the sixteen lanes that hold its slots, then over the waves in index order
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (walk == 0) {
                float v = mx[q];
                v = fmaxf(v, dpp_f32<DPP_QUAD_XOR1>(v)); v = fmaxf(v, dpp_f32<DPP_QUAD_XOR2>(v)); v = fmaxf(v, dpp_f32<DPP_HALF_MIRROR>(v)); v = fmaxf(v, dpp_f32<DPP_ROW_MIRROR>(v));
                if (r == 0) redf[wave * R + 4 * g + q] = v;
            } else {
                double v = ds[q];
                v += dpp_f64<DPP_QUAD_XOR1>(v); v += dpp_f64<DPP_QUAD_XOR2>(v); v += dpp_f64<DPP_HALF_MIRROR>(v); v += dpp_f64<DPP_ROW_MIRROR>(v);
                if (r == 0) redd[wave * R + 4 * g + q] = v;
            }
        }
        __syncthreads();
        if (tid < R) {
            if (walk == 0) rmax[tid] = fmaxf(fmaxf(redf[tid], redf[R + tid]), fmaxf(redf[2 * R + tid], redf[3 * R + tid]));
            else {
                const double sum = ((redd[tid] + redd[R + tid]) + redd[2 * R + tid]) + redd[3 * R + tid];
                rinv[tid] = sum > 0 ? (float) (1.0 / sum) : 0.f;            // (a row that sees no slot: p = 0 everywhere, zeros out)
            }
        }
        __syncthreads();
    }

    // ---- walk 3 over K and V: p into the probability tile, P x V on the f64 matrix pipe ----------------------------------------------------------
    float rm[4], ri[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { rm[q] = rmax[4 * g + q]; ri[q] = rinv[4 * g + q]; }
    f64x4_t acc[NDT];
#pragma unroll
    for (int i = 0; i < NDT; i++) acc[i] = f64x4_t{ 0, 0, 0, 0 };
    attn_q8_request<D>(regs, edge, kring, 0, tile_end(0));
    attn_q8_request<D>(vregs, vedge, vring, 0, tile_end(0));
    attn_q8_store<D>(regs, edge, buf0, kring, 0, tile_end(0));
    attn_q8_store<D>(vregs, vedge, buf1, vring, 0, tile_end(0));
    __syncthreads();
    for (int t = 0; t < NT; t++) {
        const int c0 = t * TILE, c_hi = tile_end(t);
        if (t + 1 < NT) {
            attn_q8_request<D>(regs, edge, kring, (t + 1) * TILE, tile_end(t + 1));
            attn_q8_request<D>(vregs, vedge, vring, (t + 1) * TILE, tile_end(t + 1));
        }
        attn_q8b_repack<D>(buf0, koff, kimg, kd);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; i++) {
            float sv[4];
            scores(c0, 2 * wave + i, sv);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float e = sv[q] > -INFINITY ? expf(sv[q] - rm[q]) : 0.f;
                P[(4 * g + q) * PP + 16 * (2 * wave + i) + r] = e * ri[q];
            }
        }
        __syncthreads();
        pv_steps(buf1 + voff, c_hi - c0, acc);
        __syncthreads();
        if (t + 1 < NT) {
            attn_q8_store<D>(regs, edge, buf0, kring, (t + 1) * TILE, tile_end(t + 1));
            attn_q8_store<D>(vregs, vedge, buf1, vring, (t + 1) * TILE, tile_end(t + 1));
            __syncthreads();
        }
    }
    if constexpr (OV) {   // the overlay group behind the last tile (the barrier above: the probability tile is free)
        if (wave == 0) {
            float sv[4];
            overlay_scores(sv);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float e = sv[q] > -INFINITY ? expf(sv[q] - rm[q]) : 0.f;
                P[(4 * g + q) * PP + r] = e * ri[q];
            }
        }
        __syncthreads();
        pv_steps(ov.vrows, ov.n, acc);
    }
#pragma unroll
    for (int i = 0; i < NDT; i++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = g + 4 * q;
            if (row < nrows) out[(int64_t) row * out_ts + 16 * (wave * NDT + i) + r] = (float) acc[i][q];
        }
}

bool k_attn_blocks_q8_supported(const attn_blocks_args & ba) {
    const attn_args & a = ba.a;
    const int64_t rowb = a.D / 32 * 34, al = a.D == 128 ? 8 : 4;           // (the packed ring stores: 8 bytes at D = 128, 4 at D = 64)
    if ((a.D != 64 && a.D != 128) || a.C < 1 || a.C > ATTN_Q8_MAX_C || a.H < 1 || a.k_nb1 != rowb || a.v_nb1 != rowb || a.k_nb2 % al || a.v_nb2 % al) return false;
    if (ba.n_jobs < 1 || ba.n_jobs > ATTN_BLOCKS_MAX) return false;
    for (int j = 0; j < ba.n_jobs; j++) {
        const attn_block_job & jb = ba.job[j];
        if (jb.T < 1 || jb.T > 64 || (uintptr_t) jb.kcache % al || (uintptr_t) jb.vcache % al) return false;
    }
    return true;
}
// ba.write_only selects the launch of the pair, as it does for k_attn_blocks
void k_attn_blocks_q8(hipStream_t s, const attn_blocks_args & ba) {
    const attn_args & a = ba.a;
    GGML_ASSERT(k_attn_blocks_q8_supported(ba));
    if (ba.write_only) {
        const dim3 grid((unsigned) a.H, (unsigned) ba.n_jobs);
        if (a.D == 128) attn_blocks_q8_write_kernel<128><<<grid, ATTN_Q8_THREADS, 0, s>>>(ba);
        else            attn_blocks_q8_write_kernel<64><<<grid, ATTN_Q8_THREADS, 0, s>>>(ba);
        return;
    }
    int t_max = 1;
    for (int j = 0; j < ba.n_jobs; j++) if (ba.job[j].T > t_max) t_max = ba.job[j].T;
    const dim3 grid((unsigned) ((t_max + ATTN_Q8B_ROWS - 1) / ATTN_Q8B_ROWS), (unsigned) a.H, (unsigned) ba.n_jobs);
    if (a.D == 128) attn_blocks_q8_attend_kernel<128><<<grid, ATTN_Q8_THREADS, attn_q8b_shape<128>::SMEM, s>>>(ba);   // (63.6 KB: no opt-in to larger LDS is needed)
    else            attn_blocks_q8_attend_kernel<64><<<grid, ATTN_Q8_THREADS, attn_q8b_shape<64>::SMEM, s>>>(ba);
}
