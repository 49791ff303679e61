// hip_attn_q8_rows.h - slot prefill past the ring's end over Q8_0 K / V rings (moshi_hot_config::kv_q8 = 7): the RING-ORDERED rows of one
// layer of one pass, job j = n_j <= 16 consecutive one-row attention sequences on one column of the [D, C, H, B] rings, as ONE launch -
// attn_rows_q8_kernel<D>, launcher k_attn_rows_q8. Included by hip_kernels_fused.hip behind hip_attn_q8_blocks.h, whose LDS shapes, re-packer, score
// function and three walks (attn_q8b_walks) it uses. The contract per row is hip_attn_q8.h's; the order of the rows is that of stepping them one by one.
//
// ROW-PARALLEL. k_attn_rows (BF16) walks a job's rows one after the other and streams the ring once per row. Here workgroup (head h, job j; 256 threads)
// attends with ALL n rows at once - they are the 16 query rows of the matrix instructions - and writes the ring afterwards:
//   head     the n q / k / v rows rotated and quantised (attn_q8_rope_quant). q as the blocks kernel keeps it. The n new K and V rows stay in LDS as the
//            OVERLAY: K twice - as an aligned image with its scales beside it (what the score function reads) and in ggml's row format (what the ring
//            gets) - and V in ggml's row format. slot[j] = the ring slot row j takes, read from the job's index base and stride (-1 outside the ring).
//   rule     row i must see the ring as it stands after rows 0 .. i were written and before rows i + 1 .. n - 1 are: a ring slot c comes from the OLD
//            ring bytes unless some row j <= i takes c, and then from the last such j's overlay row. Both under row i's own mask value at c. The
//            cutter's slots are (s_0 + j) mod C, for which this is "d = (c - s_0 + C) mod C: old when d >= n or d > i, else overlay row d"; the
//            kernel compares the slots themselves (the planner cannot see an uploaded index), so any assignment of slots gives stepping's result.
//   walks    attn_q8b_walks<D, true>: the blocks kernel's three walks over the old ring with the pairs (row i, slot c), c taken by a row j <= i,
//            switched off, plus the overlay as one more 16-slot group with the pairs j > i (and j >= n, and rows a later j' <= i replaces) switched
//            off - through the same score function in all three walks, so a pair's score has the same bits in each.
//   write    behind a workgroup barrier after the last walk: the overlay rows to their ring slots as packed 8- / 4-byte stores (a row whose slot a
//            later row of the job takes again is not stored: the last writer wins). Only this workgroup touches the (head, column): no fence needed.
// No workgroup waits for another, no workspace, no scratch. LDS (D = 128): the blocks kernel's layout with the probability tile laid over tile
// buffer 0 (free between the re-pack and the next tile's store in walk 3) and the overlay behind it - 61.9 KB.
#pragma once

template <int D> struct attn_q8r_shape {
    typedef attn_q8_shape<D> S;
    static constexpr int R = ATTN_Q8B_ROWS, PITCH = attn_q8b_shape<D>::PITCH;
    static constexpr int O_KIMG = 2 * S::BUF_Q8_BYTES, O_KD = O_KIMG + ATTN_Q8_TILE * PITCH, O_QQ = O_KD + ATTN_Q8_TILE * S::NBLK * 2;
    static constexpr int O_QD = O_QQ + R * PITCH, O_REDD = O_QD + R * S::NBLK * 4, O_REDF = O_REDD + 4 * R * 8, O_STAT = O_REDF + 4 * R * 4, O_REDI = O_STAT + 2 * R * 4;
    static constexpr int O_OVK = O_REDI + 16, O_OVKD = O_OVK + R * PITCH, O_KROWS = O_OVKD + R * S::NBLK * 2, O_VROWS = O_KROWS + R * S::ROWB + 8, O_SLOT = O_VROWS + R * S::ROWB + 8;
    static constexpr int SMEM = O_SLOT + R * 4;
    static_assert(R == ATTN_ROWS_Q8_MAX_N, "a job's rows are the query rows of one workgroup");
    static_assert(SMEM <= 64 * 1024 &&R * ATTN_Q8B_PP * 4 <= S::BUF_Q8_BYTES && O_KIMG % 16 == 0 && O_REDD % 8 == 0 && O_OVK % 8 == 0 && O_KROWS % 8 == 0 && O_VROWS % 8 == 0,
                  "LDS of the rows launch: under the 64 KB every launch may have, the probability tile inside tile buffer 0");
};

template <int D>
__global__ void __launch_bounds__(ATTN_Q8_THREADS) attn_rows_q8_kernel(attn_rows_args ra) {
    typedef attn_q8_shape<D> S;
    typedef attn_q8r_shape<D> L;
    constexpr int NBLK = S::NBLK, ROWB = S::ROWB, half = D / 2, PITCH = L::PITCH, R = L::R, LPR = D / 4, PIECE = D == 128 ? 8 : 4, NPC = ROWB / PIECE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const attn_rows_job & jb = ra.job[blockIdx.y];
    const attn_args & a = ra.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int h = blockIdx.x, C = a.C, n = jb.n;

    char * qq = smem + L::O_QQ; float * qd = (float *) (smem + L::O_QD);
    float * rmax = (float *) (smem + L::O_STAT);
    int * redi = (int *) (smem + L::O_REDI);
    char * ovk = smem + L::O_OVK; uint16_t * ovkd = (uint16_t *) (smem + L::O_OVKD);
    char * krows = smem + L::O_KROWS, * vrows = smem + L::O_VROWS;
    int * slot = (int *) (smem + L::O_SLOT);
    char * kring = jb.kcache + (int64_t) h * a.k_nb2, * vring = jb.vcache + (int64_t) h * a.v_nb2;

    // ---- head: the ring slots; the q / k / v rows, rotated and quantised (unit = kind * 16 + row; a row past n is zeros with scale 0) -------------------
    if (tid < R) {
        const int s = tid < n ? *(const int32_t *) (jb.index + tid * jb.index_rs) : -1;
        slot[tid] = s >= 0 && s < C ? s : -1;
    }
#pragma unroll
    for (int pass = 0; pass < 3 * R * LPR / ATTN_Q8_THREADS; pass++) {
        const int u = pass * ATTN_Q8_THREADS + tid, unit = u / LPR, kind = unit / R, row = unit % R, ln = u % LPR, j0 = ln * 4;   // kind 0: q, 1: k, 2: v
        float in0[4], in1[4], rc[4], rs[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { in0[i] = 0.f; in1[i] = 0.f; rc[i] = 1.f; rs[i] = 0.f; }
        const bool rotate = kind < 2 && jb.rot;
        if (row < n) {
            const float * src = kind == 0 ? (const float *) (jb.q + row * jb.q_rs) + (int64_t) h * a.q_hs
                              : kind == 1 ? (const float *) (jb.k + row * jb.k_rs) + (int64_t) h * a.k_hs : (const float *) (jb.v + row * jb.v_rs) + (int64_t) h * a.v_hs;
            if (rotate) {
                const float * rot = (const float *) (jb.rot + row * jb.rot_rs);
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
        if (kind == 0) {
            *(uint32_t *) (qq + row * PITCH + j0) = packed;
            if ((ln & 7) == 0) qd[row * NBLK + (ln >> 3)] = h2f(dh);
        } else {
            if (kind == 1) {
                *(uint32_t *) (ovk + row * PITCH + j0) = packed;
                if ((ln & 7) == 0) ovkd[row * NBLK + (ln >> 3)] = dh;
            }
            char * blk = (kind == 1 ? krows : vrows) + row * ROWB + (ln >> 3) * 34;   // block ln / 8: d, then the quants 2 bytes in
            uint16_t * qs = (uint16_t *) (blk + 2 + (ln & 7) * 4);
            qs[0] = (uint16_t) (packed & 0xffff); qs[1] = (uint16_t) (packed >> 16);
            if ((ln & 7) == 0) *(uint16_t *) blk = dh;
        }
    }
    {   // the live end over the job's rows: the largest un-masked slot of any of them
        int last = -1;
        const int row = tid >> 4;
        if (row < n) {
            const float * mr = (const float *) (jb.mask + row * jb.mask_rs);
            for (int c = tid & 15; c < C; c += 16) if (mr[c] > -INFINITY) last = c;   // (ascending c: the last hit is the largest)
        }
        last = wave_allmax_i32(last);
        if (lane == 0) redi[wave] = last;
    }
    __syncthreads();
    const int n_end = max(max(redi[0], redi[1]), max(redi[2], redi[3])) + 1;

    // ---- attend: all rows at once, over the old ring and the overlay --------------------------------------------------------------------------------
    if (n_end <= 0) {   // no row sees a slot: zeros
        for (int i = tid; i < n * D; i += ATTN_Q8_THREADS) ((float *) (jb.out + (i / D) * jb.out_rs))[h * D + i % D] = 0.f;
    } else {
        const float * mrow[4];
#pragma unroll
        for (int q = 0; q < 4; q++) mrow[q] = 4 * g + q < n ? (const float *) (jb.mask + (4 * g + q) * jb.mask_rs) : nullptr;
        const attn_q8b_lds m = { smem, smem + S::BUF_Q8_BYTES, smem + L::O_KIMG, (uint16_t *) (smem + L::O_KD), (float *) smem, qq, qd,
                                 (double *) (smem + L::O_REDD), (float *) (smem + L::O_REDF), rmax, rmax + R };
        attn_q8b_overlay ov;
        ov.kimg = ovk; ov.kd = ovkd; ov.vrows = vrows; ov.slot = slot; ov.n = n;
        attn_q8b_walks<D, true>(m, ov, kring, vring, mrow, n, n_end, C, a.scale, (float *) jb.out + (int64_t) h * D, jb.out_rs / 4);
    }

    // ---- write: the overlay rows to their ring slots, packed; the last row that takes a slot wins ------------------------------------------------------
    __syncthreads();
    for (int p = tid; p < 2 * n * NPC; p += ATTN_Q8_THREADS) {
        const int pu = p / NPC, pc = p % NPC, kv = pu >= n, j = pu - kv * n, s = slot[j];
        bool stays = s >= 0;
        for (int j2 = j + 1; j2 < n; j2++) stays = stays && slot[j2] != s;
        if (!stays) continue;
        char * dst = (kv ? vring + (int64_t) s * a.v_nb1 : kring + (int64_t) s * a.k_nb1) + pc * PIECE;
        const char * from = (kv ? vrows : krows) + j * ROWB + pc * PIECE;
        if (D == 128) *(uint2 *) dst = *(const uint2 *) from; else *(uint32_t *) dst = *(const uint32_t *) from;
    }
}

bool k_attn_rows_q8_supported(const attn_rows_args & ra) {
    const attn_args & a = ra.a;
    const int64_t rowb = a.D / 32 * 34, al = a.D == 128 ? 8 : 4;           // (the packed ring stores: 8 bytes at D = 128, 4 at D = 64)
    if ((a.D != 64 && a.D != 128) || a.C < 1 || a.C > ATTN_Q8_MAX_C || a.H < 1 || a.k_nb1 != rowb || a.v_nb1 != rowb || a.k_nb2 % al || a.v_nb2 % al) return false;
    if (ra.n_jobs < 1 || ra.n_jobs > ATTN_ROWS_MAX) return false;
    for (int j = 0; j < ra.n_jobs; j++) {
        const attn_rows_job & jb = ra.job[j];
        if (jb.n < 2 || jb.n > ATTN_Q8B_ROWS || jb.n > a.C || (uintptr_t) jb.kcache % al || (uintptr_t) jb.vcache % al) return false;
        for (int64_t rs : { jb.q_rs, jb.k_rs, jb.v_rs, jb.mask_rs, jb.rot_rs, jb.index_rs, jb.out_rs }) if (rs % 4) return false;
    }
    return true;
}
void k_attn_rows_q8(hipStream_t s, const attn_rows_args & ra) {
    const attn_args & a = ra.a;
    GGML_ASSERT(k_attn_rows_q8_supported(ra));
    const dim3 grid((unsigned) a.H, (unsigned) ra.n_jobs);
    if (a.D == 128) attn_rows_q8_kernel<128><<<grid, ATTN_Q8_THREADS, attn_q8r_shape<128>::SMEM, s>>>(ra);   // (61.9 KB: no opt-in to larger LDS is needed)
    else            attn_rows_q8_kernel<64><<<grid, ATTN_Q8_THREADS, attn_q8r_shape<64>::SMEM, s>>>(ra);
}
