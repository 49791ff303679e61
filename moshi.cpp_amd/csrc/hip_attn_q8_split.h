// hip_attn_q8_split.h - the single-token self-attention block of B columns over Q8_0 K / V rings (hip_attn_q8.h) with every (head, column)
// split along the ring over S workgroups: a launch PAIR of S x H x B workgroups each, attn_q8_split_scores_kernel<D> and
// attn_q8_split_values_kernel<D>, launcher k_attn_streams_q8_split. Included by hip_kernels_fused.hip behind hip_attn_q8.h, whose pieces it uses: the
// shape, the tile request / store, the RoPE + quantiser, the score lane map and the P x V lane map.
//
// WHY: attn_streams_q8_kernel is H x B workgroups, each walking its whole live ring alone. At few columns and a long ring (H x B well under the CU
// count, some hundred to 4096 live slots) most of the device idles while a head streams its ring at one CU's rate. Here the ring walk of a head is cut
// into S contiguous slices. The launch boundary is the only ordering between scores and values; inside a launch NO workgroup waits for another (no flag
// is polled, nothing spins), so residency does not matter.
//
// CHUNKS. The live range [0, n_end) - n_end found from the column's whole mask row by every workgroup of both launches, as attn_streams_q8_kernel finds
// it - is cut into chunks of ATTN_Q8_SPLIT_CHUNK slots (whole tiles). Slice s of S owns a contiguous, balanced run of whole chunks (attn_q8_slice: the
// first n_chunks % S slices hold one chunk more); slices beyond the last chunk are empty.
//
// LAUNCH 1, scores (workgroup (s, h, b)): the head stage of attn_streams_q8_kernel - q and k rotated and quantised by every workgroup (a head row is D
//   floats: recomputing costs less than exchanging); workgroup s == 0 also quantises v and stores the new k / v rows to their ring slot. Then the K tiles
//   of the slice through the two LDS buffers, one barrier per tile, scores by the (slot, block) lane map. The slot written this step is taken from the
//   workgroup's own LDS copy of the new k row (last writer wins), so the concurrent ring store by s == 0 is never observed. The masked, scaled scores of
//   the slice go to scores[b][h][c] in the workspace, -inf for masked slots. Every slot of [0, n_end) belongs to exactly one slice.
// LAUNCH 2, values (workgroup (s, h, b)): all n_end scores of the (head, column) into LDS and attn_streams_q8_kernel's soft_max over them - the same
//   loops and reduction order, so p has that kernel's bits in every slice. Then the V tiles of the slice by the (g, lc) lane map; every V row, the new
//   one included, comes from the ring (launch 1 wrote it). The eight double accumulators of a thread start at zero at every CHUNK; after the chunk's last
//   tile the G partial rows are reduced - group g and group g + G / 8, which share a wave, through a lane exchange, then the G / 2 rows in LDS in index
//   order - and the chunk's D doubles go to part[b][h][chunk][0 .. D) with returning agent-scope exchanges. The workgroup then draws a ticket from the
//   (head, column)'s arrival counter; the LAST to arrive (empty slices arrive too) adds the chunk rows in chunk order in double, writes out as float -
//   zeros for an empty row - and puts the counter back to zero for the next launch or hipGraph replay. Publication and merge are those of
//   vq_level_cols_kernel: xchg_agent_wait, barrier, atomicAdd, agent-coherent loads.
//
// NUMERICS. Ring bytes, scores and p are attn_streams_q8_kernel's. The output is the sum over chunks, in chunk order, of the chunk sums; it differs from
// the unsplit kernel's in the grouping of the double sums alone (DESIGN.md 35's bar holds). Partials are per CHUNK, not per slice: a column's bits depend
// on its own values only - not on S, B, the CU count or its neighbours.
#pragma once

#define ATTN_Q8_SPLIT_CHUNK 256   // ring slots per partial sum: whole tiles
#define ATTN_Q8_SPLIT_MAX 16      // slices per (head, column) at most
static_assert(ATTN_Q8_SPLIT_CHUNK % ATTN_Q8_TILE == 0, "a chunk is whole tiles");

__host__ __device__ static inline int attn_q8_split_chunks(int n) { return (n + ATTN_Q8_SPLIT_CHUNK - 1) / ATTN_Q8_SPLIT_CHUNK; }
template <int D> static size_t attn_q8_split_values_smem(int C) {
    typedef attn_q8_shape<D> S;
    return (((size_t) C * 4 + 15) & ~(size_t) 15) + 2 * S::BUF_Q8_BYTES + (size_t) (S::G / 2) * D * 8;   // probabilities | two tile buffers | G / 2 partial rows
}

// the live range's end of a mask row: its last un-masked slot + 1 (0: an empty or closed column). With `sc` the row is also staged there. Ends in a barrier.
__device__ __forceinline__ int attn_q8_live_end(const float * mask, int C, float * sc, int * sh_i) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NMASK = ATTN_Q8_MAX_C / ATTN_Q8_THREADS;
    float mpre[NMASK];
#pragma unroll
    for (int i = 0; i < NMASK; i++) { const int c = tid + i * ATTN_Q8_THREADS; mpre[i] = mask[c < C ? c : C - 1]; }
    int last = -1;
#pragma unroll
    for (int i = 0; i < NMASK; i++) {
        const int c = tid + i * ATTN_Q8_THREADS;
        if (c < C) { if (sc) sc[c] = mpre[i]; if (mpre[i] > -INFINITY) last = c; }   // (ascending c: the last hit is the largest)
    }
    last = wave_allmax_i32(last);
    if (lane == 0) sh_i[wave] = last;
    __syncthreads();
    return max(max(sh_i[0], sh_i[1]), max(sh_i[2], sh_i[3])) + 1;
}
// the chunks [k0, k1) of slice s of S over a live range of n_end slots
__device__ __forceinline__ void attn_q8_slice(int n_end, int s, int S, int & k0, int & k1) {
    const int nch = n_end > 0 ? (n_end + ATTN_Q8_SPLIT_CHUNK - 1) / ATTN_Q8_SPLIT_CHUNK : 0, q = nch / S, r = nch % S;
    k0 = s * q + (s < r ? s : r);
    k1 = k0 + q + (s < r ? 1 : 0);
}

template <int D>
__global__ void __launch_bounds__(ATTN_Q8_THREADS) attn_q8_split_scores_kernel(attn_streams_args sa, float * scores) {
    typedef attn_q8_shape<D> S;
    constexpr int NBLK = S::NBLK, ROWB = S::ROWB, TILE = ATTN_Q8_TILE, half = D / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int sh_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, h = blockIdx.y;
    const int64_t b = blockIdx.z;
    const attn_args & a = sa.a;
    const int C = a.C;

    float * sc = (float *) smem;                                            // [C] the mask row
    char * p_ = smem + (((size_t) C * 4 + 15) & ~(size_t) 15);
    int8_t * qq = (int8_t *) p_; p_ += D;                                   // the quantised query ...
    float * qd = (float *) p_; p_ += 16;                                    // ... and its block scales
    char * knew = p_; p_ += S::ROW_Q8_BUF;                                  // the new K / V rows in ggml's row format
    char * vnew = p_; p_ += S::ROW_Q8_BUF;
    char * const buf0 = p_;                                                 // the two tile buffers, 16-byte aligned
    auto buf_of = [&](int t) { return buf0 + (t & 1) * S::BUF_Q8_BYTES; };

    const float * mask = a.mask + b * sa.mask_bs;
    const char * kring = a.kcache + b * sa.kc_bs + (int64_t) h * a.k_nb2;
    const char * vring = a.vcache + b * sa.vc_bs + (int64_t) h * a.v_nb2;
    float * srow = scores + (b * gridDim.y + h) * C;

    // ---- head: q and k in every workgroup, v in the one that stores the new rows ------------------------------------------------------------------
    const int slot = a.index[b * sa.index_bs];
    const int n_rows = s == 0 ? 3 : 2;                                      // wave 0: q, 1: k, 2: v
    float in0[4], in1[4], rc[4], rs[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { in0[i] = 0.f; in1[i] = 0.f; rc[i] = 1.f; rs[i] = 0.f; }
    const bool row_lane = wave < n_rows && lane < D / 4;                   // lane: outputs 4 lane .. 4 lane + 3
    const int j0 = lane * 4;
    if (row_lane) {
        const float * src = wave == 0 ? a.q + b * sa.q_bs + (int64_t) h * a.q_hs : wave == 1 ? a.k + b * sa.k_bs + (int64_t) h * a.k_hs : a.v + b * sa.v_bs + (int64_t) h * a.v_hs;
        if (wave < 2 && a.rot) {
            const float * rot = a.rot + b * sa.rot_bs;
            const int p0 = j0 < half ? j0 : j0 - half;
#pragma unroll
            for (int i = 0; i < 4; i++) { in0[i] = src[2 * (p0 + i)]; in1[i] = src[2 * (p0 + i) + 1]; rc[i] = rot[p0 + i]; rs[i] = rot[half + p0 + i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) in0[i] = src[j0 + i];
        }
    }
    if (wave < n_rows) {
        uint16_t dh;
        const uint32_t packed = attn_q8_rope_quant(in0, in1, rc, rs, wave < 2 && a.rot, j0 >= half, dh);
        if (row_lane) {
            if (wave == 0) {
                *(uint32_t *) (qq + j0) = packed;
                if ((lane & 7) == 0) qd[lane >> 3] = h2f(dh);
            } else {
                char * row = (wave == 1 ? knew : vnew) + (lane >> 3) * 34;  // block lane / 8: d, then the quants 2 bytes in
                uint16_t * qs = (uint16_t *) (row + 2 + (lane & 7) * 4);
                qs[0] = (uint16_t) (packed & 0xffff); qs[1] = (uint16_t) (packed >> 16);
                if ((lane & 7) == 0) *(uint16_t *) row = dh;
            }
        }
    }
    const int n_end = attn_q8_live_end(mask, C, sc, sh_i);                  // (its barrier: q, the new rows and the mask row are in LDS)

    // the new rows go to their ring slot from LDS, packed - one workgroup of the head's S
    if (s == 0 && slot >= 0 && slot < C) {
        if (D == 128) {
            if (tid < ROWB / 8) *(uint2 *) (const_cast<char *>(kring) + (int64_t) slot * a.k_nb1 + tid * 8) = *(const uint2 *) (knew + tid * 8);
            else if (tid >= 64 && tid < 64 + ROWB / 8) *(uint2 *) (const_cast<char *>(vring) + (int64_t) slot * a.v_nb1 + (tid - 64) * 8) = *(const uint2 *) (vnew + (tid - 64) * 8);
        } else {
            if (tid < ROWB / 4) *(uint32_t *) (const_cast<char *>(kring) + (int64_t) slot * a.k_nb1 + tid * 4) = *(const uint32_t *) (knew + tid * 4);
            else if (tid >= 64 && tid < 64 + ROWB / 4) *(uint32_t *) (const_cast<char *>(vring) + (int64_t) slot * a.v_nb1 + (tid - 64) * 4) = *(const uint32_t *) (vnew + (tid - 64) * 4);
        }
    }
    int k0, k1;
    attn_q8_slice(n_end, s, (int) gridDim.x, k0, k1);
    if (k0 >= k1) return;                                                   // an empty slice (or an empty row: launch 2 writes its zeros)
    const int c_lo = k0 * ATTN_Q8_SPLIT_CHUNK, c_hi = min(k1 * ATTN_Q8_SPLIT_CHUNK, n_end);
    const int t0 = c_lo / TILE, t1 = (c_hi + TILE - 1) / TILE;
    auto tile_end = [&](int t) { const int e = (t + 1) * TILE; return e < c_hi ? e : c_hi; };
    // byte offset from smem of slot c of tile t in its buffer - or, for the slot written this step, of the new row
    auto slot_offset = [&](int t, int c) {
        const int off0 = (int) ((uintptr_t) (kring + (int64_t) t * TILE * ROWB) & 15);
        return c == slot ? (int) (knew - smem) : (int) (buf_of(t) - smem) + off0 + (c - t * TILE) * ROWB;
    };

    attn_q8_u32x4 regs[S::NPIECE];   // a tile's pieces between their request and their store to LDS
    uint32_t edge;
    attn_q8_request<D>(regs, edge, kring, c_lo, tile_end(t0));
    constexpr int LPS = NBLK, SPP = ATTN_Q8_THREADS / LPS;                // lanes per slot, slots per pass
    const int blk = tid % LPS, sp = tid / LPS;
    int qreg[8];
#pragma unroll
    for (int i = 0; i < 8; i++) qreg[i] = ((const int *) (qq + blk * 32))[i];
    const float dq = qd[blk];
    attn_q8_store<D>(regs, edge, buf_of(t0), kring, c_lo, tile_end(t0));
    __syncthreads();
    for (int t = t0; t < t1; t++) {
        if (t + 1 < t1) attn_q8_request<D>(regs, edge, kring, (t + 1) * TILE, tile_end(t + 1));
        const int ce = tile_end(t);
#pragma unroll
        for (int pass = 0; pass < TILE / SPP; pass++) {
            const int c = t * TILE + pass * SPP + sp, cc = c < ce ? c : ce - 1;
            const int A = slot_offset(t, cc) + blk * 34;                    // the block: even, not always a dword boundary
            const uint32_t * w = (const uint32_t *) (smem + (A & ~3));
            const bool odd = (A & 2) != 0;
            uint32_t wv[9];
#pragma unroll
            for (int i = 0; i < 9; i++) wv[i] = w[i];
            const float dk = h2f((uint16_t) (odd ? wv[0] >> 16 : wv[0] & 0xffff));
            int sumi = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t kq = odd ? wv[i + 1] : __builtin_amdgcn_alignbyte(wv[i + 1], wv[i], 2);
                sumi = dot4_i8((int) kq, qreg[i], sumi);
            }
            const float term = (float) sumi * (dk * dq);
            float sumf = 0.f;
            if (NBLK == 4) {
                sumf += attn_q8_quad<0x00>(term); sumf += attn_q8_quad<0x55>(term); sumf += attn_q8_quad<0xAA>(term); sumf += attn_q8_quad<0xFF>(term);
            } else {
                sumf += attn_q8_quad<0xA0>(term); sumf += attn_q8_quad<0xF5>(term);   // quad_perm [0, 0, 2, 2] and [1, 1, 3, 3]: the slot's two blocks
            }
            if (c < ce && blk == 0) {
                const float m = sc[c];
                float sv = -INFINITY;
                if (m > -INFINITY) { sv = sumf * a.scale; sv = sv + m; }
                srow[c] = sv;
            }
        }
        if (t + 1 < t1) attn_q8_store<D>(regs, edge, buf_of(t + 1), kring, (t + 1) * TILE, tile_end(t + 1));
        __syncthreads();
    }
}

template <int D>
__global__ void __launch_bounds__(ATTN_Q8_THREADS) attn_q8_split_values_kernel(attn_streams_args sa, const float * scores, double * part, unsigned * counters) {
    typedef attn_q8_shape<D> S;
    constexpr int ROWB = S::ROWB, TILE = ATTN_Q8_TILE, LC = S::LC, G = S::G, GH = 32 / LC;   // GH: the slot groups of half a wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float sh_f[4];
    __shared__ double sh_d[4];
    __shared__ int sh_i[4];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, h = blockIdx.y;
    const int64_t b = blockIdx.z;
    const attn_args & a = sa.a;
    const int C = a.C;

    float * sc = (float *) smem;                                            // [C] scores -> exponentials -> probabilities
    char * const buf0 = smem + (((size_t) C * 4 + 15) & ~(size_t) 15);      // the two tile buffers, 16-byte aligned
    auto buf_of = [&](int t) { return buf0 + (t & 1) * S::BUF_Q8_BYTES; };
    double * red = (double *) (buf0 + 2 * S::BUF_Q8_BYTES);                 // [G / 2][D] partial rows of a chunk

    const char * vring = a.vcache + b * sa.vc_bs + (int64_t) h * a.v_nb2;
    const int64_t bh = b * gridDim.y + h;
    const float * srow = scores + bh * C;
    double * prow = part + bh * attn_q8_split_chunks(C) * D;

    const int n_end = attn_q8_live_end(a.mask + b * sa.mask_bs, C, nullptr, sh_i);
    int k0, k1;
    attn_q8_slice(n_end, s, (int) gridDim.x, k0, k1);
    if (k0 < k1) {
        const int c_lo = k0 * ATTN_Q8_SPLIT_CHUNK, c_hi = min(k1 * ATTN_Q8_SPLIT_CHUNK, n_end);
        const int t0 = c_lo / TILE, t1 = (c_hi + TILE - 1) / TILE;
        auto tile_end = [&](int t) { const int e = (t + 1) * TILE; return e < c_hi ? e : c_hi; };
        attn_q8_u32x4 regs[S::NPIECE];
        uint32_t edge;
        attn_q8_request<D>(regs, edge, vring, c_lo, tile_end(t0));         // the first V tile is on its way during the soft_max

        // ---- soft_max over the whole live range: attn_streams_q8_kernel's, to the letter ------------------------------------------------------
        float lmax = -INFINITY;
        for (int c = tid; c < n_end; c += ATTN_Q8_THREADS) { const float sv = srow[c]; sc[c] = sv; lmax = fmaxf(lmax, sv); }
        lmax = wave_allmax_f32(lmax);
        if (lane == 0) sh_f[wave] = lmax;
        __syncthreads();
        const float gmax = fmaxf(fmaxf(sh_f[0], sh_f[1]), fmaxf(sh_f[2], sh_f[3]));
        double lsum = 0;
        for (int c = tid; c < n_end; c += ATTN_Q8_THREADS) {
            const float sv = sc[c];
            const float e = sv > -INFINITY ? expf(sv - gmax) : 0.f;
            sc[c] = e;
            lsum += (double) e;
        }
        lsum = wave_allsum_f64(lsum);
        if (lane == 0) sh_d[wave] = lsum;
        __syncthreads();
        const float inv = (float) (1.0 / (((sh_d[0] + sh_d[1]) + sh_d[2]) + sh_d[3]));
        for (int c = tid; c < n_end; c += ATTN_Q8_THREADS) sc[c] = sc[c] * inv;
        attn_q8_store<D>(regs, edge, buf_of(t0), vring, c_lo, tile_end(t0));
        __syncthreads();

        // ---- P x V, a partial row per chunk ----------------------------------------------------------------------------------------------------
        const int lc = tid % LC, g = tid / LC;
        for (int k = k0; k < k1; k++) {
            double acc[8];
#pragma unroll
            for (int i = 0; i < 8; i++) acc[i] = 0;
            const int te = min((k + 1) * (ATTN_Q8_SPLIT_CHUNK / TILE), t1);
            for (int t = k * (ATTN_Q8_SPLIT_CHUNK / TILE); t < te; t++) {
                if (t + 1 < t1) attn_q8_request<D>(regs, edge, vring, (t + 1) * TILE, tile_end(t + 1));
                const int ce = tile_end(t);
                const int base = (int) (buf_of(t) - smem) + (int) ((uintptr_t) (vring + (int64_t) t * TILE * ROWB) & 15);
                for (int c = t * TILE + g; c < ce; c += G) {
                    const float p = sc[c];
                    const int A = base + (c - t * TILE) * ROWB + (lc >> 2) * 34;   // the block of dims 8 lc ..
                    const int Q = A + 2 + (lc & 3) * 8;                            // .. and their eight quants
                    const float dv = h2f(*(const uint16_t *) (smem + A));
                    const uint32_t * w = (const uint32_t *) (smem + (Q & ~3));
                    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
                    const bool odd = (Q & 2) != 0;
                    const uint32_t lo = odd ? __builtin_amdgcn_alignbyte(w1, w0, 2) : w0, hi = odd ? __builtin_amdgcn_alignbyte(w2, w1, 2) : w1;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const float v0 = dv * (float) (int8_t) (lo >> (8 * i)), v1 = dv * (float) (int8_t) (hi >> (8 * i));
                        acc[i] += (double) (v0 * p);
                        acc[4 + i] += (double) (v1 * p);
                    }
                }
                if (t + 1 < t1) attn_q8_store<D>(regs, edge, buf_of(t + 1), vring, (t + 1) * TILE, tile_end(t + 1));
                __syncthreads();
            }
            // the chunk's row: group g + group g + GH inside the wave, then the G / 2 rows in index order (red is free: its readers of the
            // previous chunk have passed a tile barrier since)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const double other = __shfl_xor(acc[i], 32, 64);
                if (lane < 32) red[(wave * GH + lane / LC) * D + lc * 8 + i] = acc[i] + other;
            }
            __syncthreads();
            if (tid < D) {
                double tot = 0;
                for (int r = 0; r < G / 2; r++) tot += red[r * D + tid];
                xchg_agent_wait(prow + (int64_t) k * D + tid, tot);         // complete before the counter moves
            }
        }
    }
    // ---- arrival: the last workgroup of the (head, column) adds the chunk rows in chunk order ------------------------------------------------------
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(counters + bh, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!s_last) return;
    if (tid < D) {
        const int nch = n_end > 0 ? attn_q8_split_chunks(n_end) : 0;
        double tot = 0;
        for (int k = 0; k < nch; k++) tot += ld_agent(prow + (int64_t) k * D + tid);
        a.out[b * sa.out_bs + (int64_t) h * D + tid] = (float) tot;        // (an empty row: zeros, as the unsplit kernel writes)
    }
    if (tid == 0) counters[bh] = 0u;
}

// workspace: arrival counters [B x H] (256-byte granule) | part [B x H x chunks(C) x D] doubles | scores [B x H x C] floats
static size_t attn_q8_split_counter_bytes(const attn_streams_args & sa) { return (((size_t) sa.B * sa.a.H * 4) + 255) & ~(size_t) 255; }
static size_t attn_q8_split_part_bytes(const attn_streams_args & sa) { return (size_t) sa.B * sa.a.H * attn_q8_split_chunks(sa.a.C) * sa.a.D * 8; }
size_t k_attn_streams_q8_split_ws_size(const attn_streams_args & sa) {
    return attn_q8_split_counter_bytes(sa) + attn_q8_split_part_bytes(sa) + (size_t) sa.B * sa.a.H * sa.a.C * 4;
}
bool k_attn_streams_q8_split_supported(const attn_streams_args & sa) {
    return k_attn_streams_q8_supported(sa) && sa.a.H <= 65535 && sa.B <= 65535;   // (grid y and z)
}
// how many slices a (head, column) of this block takes under the handle's setting (ggml_backend_mi355x_set_attn_q8_split): 0 / 1: the unsplit launch
int k_attn_streams_q8_split_slices(const attn_streams_args & sa, int setting, int usable_cus) {
    if (setting <= 0 || !k_attn_streams_q8_split_supported(sa)) return 0;
    const int nch = attn_q8_split_chunks(sa.a.C);
    int S = setting == 1 ? usable_cus / (int) (sa.a.H * sa.B) : setting;   // auto: one workgroup per compute unit
    S = S < nch ? S : nch;
    return S < ATTN_Q8_SPLIT_MAX ? S : ATTN_Q8_SPLIT_MAX;
}
void k_attn_streams_q8_split(hipStream_t st, const attn_streams_args & sa, int S, void * ws, int launch) {
    const attn_args & a = sa.a;
    GGML_ASSERT(k_attn_streams_q8_split_supported(sa) && ws && S >= 2 && S <= ATTN_Q8_SPLIT_MAX && S <= attn_q8_split_chunks(a.C));
    const size_t smem1 = a.D == 128 ? attn_q8_smem<128>(a.C) : attn_q8_smem<64>(a.C);
    const size_t smem2 = a.D == 128 ? attn_q8_split_values_smem<128>(a.C) : attn_q8_split_values_smem<64>(a.C);
    GGML_ASSERT(smem1 <= 64 * 1024 && smem2 <= 64 * 1024);                 // (C <= 4096: 51.7 KB and 58.1 KB at D = 128 - no opt-in to larger LDS is needed)
    unsigned * counters = (unsigned *) ws;
    double * part = (double *) ((char *) ws + attn_q8_split_counter_bytes(sa));
    float * scores = (float *) ((char *) part + attn_q8_split_part_bytes(sa));
    const dim3 grid((unsigned) S, (unsigned) a.H, (unsigned) sa.B);
    if (launch != 1) {   // scores
        if (a.D == 128) attn_q8_split_scores_kernel<128><<<grid, ATTN_Q8_THREADS, smem1, st>>>(sa, scores);
        else            attn_q8_split_scores_kernel<64><<<grid, ATTN_Q8_THREADS, smem1, st>>>(sa, scores);
    }
    if (launch != 0) {   // values
        if (a.D == 128) attn_q8_split_values_kernel<128><<<grid, ATTN_Q8_THREADS, smem2, st>>>(sa, scores, part, counters);
        else            attn_q8_split_values_kernel<64><<<grid, ATTN_Q8_THREADS, smem2, st>>>(sa, scores, part, counters);
    }
}
