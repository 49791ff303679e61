// hip_attn_q8.h - the single-token self-attention block of B columns over Q8_0 K / V rings (moshi_hot_config::kv_q8): ONE launch of
// H x B workgroups, attn_streams_q8_kernel<D>, launcher k_attn_streams_q8. Included by hip_kernels_fused.hip.
//
// THE BLOCK (attention() in moshi_hot.cpp with Q8_0 rings): k = set_rows(kcache, rope(k)), v = set_rows(vcache, v), w = soft_max(mul_mat(k, q) * scale +
// mask), o = mul_mat(cont(transpose(get_rows(v, iota))), w). ggml's arithmetic for these nodes is the contract:
//   ring row   quantize_row_q8_0 of the F32 row: per 32 values d = amax / 127 kept as F16, q = roundf(x * (d ? 1 / d : 0))
//   score      vec_dot_q8_0_q8_0: the query row quantised the same way; per block the exact integer dot times float(h2f(d_k) * h2f(d_q)); the D / 32
//              block terms added in float, in block order
//   soft_max   x = score * scale + mask in float, maximum, exponentials summed in double, p = e * float(1 / sum) - p is NOT rounded (P x V is F32 x F32)
//   output     out[d] = float(sum over slots of double(float(v) * p)), v = h2f(d_v) * q_v (exact in float), in double
//
// THE WORKGROUP (head h, column b; 256 threads = 4 waves; nobody waits for another workgroup, no workspace, no scratch):
//   head       every load that depends on no computed value goes out first: the ring slot, the new q / k / v rows and the RoPE row (wave 0: q, 1: k,
//              2: v - a lane holds 4 consecutive outputs, 8 lanes a block of 32), the mask row (all threads), the first K tile. q and k are rotated as
//              apply_rope does, the three rows quantised (quantize_block_q80's arithmetic: amax of a block over 8 lanes by DPP). q stays in LDS as
//              D int8 + D / 32 scales; k and v stay in LDS in ggml's row format (blocks of 34 bytes) and go to the ring slot as packed stores from
//              there (8 bytes each at D = 128, a row being 136 = 17 x 8; 4 bytes at D = 64, a row being 68). The mask row is staged in the score
//              buffer; the last un-masked slot ends the live range [0, n_end). An empty row writes zeros (what the BF16 body writes).
//   ring walk  a head's ring column is one contiguous run of C x ROWB bytes whose rows and blocks are only 4- / 2-byte aligned, so it is never read
//              block by block from HBM: a TILE of 128 slots (17 408 bytes at D = 128) is copied as raw bytes - dword pieces up to the first 16-byte
//              boundary, 16-byte pieces, dword pieces for the tail; no byte outside the tile's range is touched - through registers into one of two LDS
//              buffers, keeping its alignment modulo 16. Tile t + 1 is requested before tile t is consumed and stored behind it: one barrier per tile.
//              Every ring byte of the live range crosses HBM once for K and once for V. The slot written this step is read from the LDS copy of the
//              new row (last writer wins), never from the tile.
//   scores     a lane owns (slot, block): D / 32 lanes per slot, 256 / (D / 32) slots per pass. It reads its block's nine dwords from LDS, byte-aligns
//              them where the block starts on an odd halfword (v_alignbyte_b32), forms the integer dot with eight v_dot4_i32_i8 against the query
//              block it holds in registers and scales it. The block terms of a slot are gathered inside its quad by DPP and added in block order by
//              every lane of the slot; lane 0 of the slot stores the masked, scaled score.
//   soft_max   over the scores in LDS: block maximum, expf, double sum (lanes stride the range, then waves in index order), p = e * float(1 / sum).
//   P x V      a second walk over the V tiles. Thread (g, lc): slot group g of G = 256 / (D / 8), dims 8 lc .. 8 lc + 7 (a quarter block). It adds
//              double(float(v) * p) over the slots g, g + G, g + 2 G ... of the live range in ascending order into eight accumulators; the G partial
//              rows go to LDS (over the tile buffers) and dim j is their sum in group order g = 0 .. G - 1.
//   A column's bits depend on its own values only: nothing here looks at B or at another column.
#pragma once

#define ATTN_Q8_THREADS 256
#define ATTN_Q8_TILE 128          // ring slots per LDS tile
#define ATTN_Q8_MAX_C 4096
typedef unsigned int attn_q8_u32x4 __attribute__((ext_vector_type(4)));

template <int D> struct attn_q8_shape {
    static constexpr int NBLK = D / 32, ROWB = NBLK * 34;                 // bytes of a ring row
    static constexpr int TILE_Q8_BYTES = ATTN_Q8_TILE * ROWB;
    static constexpr int BUF_Q8_BYTES = TILE_Q8_BYTES + 48;                     // 16: the tile's alignment offset; the rest: reads of whole dwords past the last block
    static constexpr int NPIECE = (TILE_Q8_BYTES / 16 + ATTN_Q8_THREADS - 1) / ATTN_Q8_THREADS;   // 16-byte pieces per thread
    static constexpr int ROW_Q8_BUF = (ROWB + 8 + 15) & ~15;                 // a new row in LDS, with the same slack
    static constexpr int LC = D / 8, G = ATTN_Q8_THREADS / LC;            // P x V: lanes per slot, slot groups
};
template <int D> static size_t attn_q8_smem(int C) {
    typedef attn_q8_shape<D> S;
    return (((size_t) C * 4 + 15) & ~(size_t) 15) + D + 16 + 2 * S::ROW_Q8_BUF + 2 * S::BUF_Q8_BYTES;   // (the G x D doubles of the final sums lie over the tile buffers)
}

// request the bytes of slots [c0, c1) of the ring column at `ring`. Threads 0 .. 2 take the dwords in front of the first 16-byte boundary, threads
// 64 .. 66 those behind the last one; every thread takes NPIECE 16-byte pieces (a thread without a piece asks for the last one again, which is not stored).
template <int D> __device__ __forceinline__ void attn_q8_request(attn_q8_u32x4 (&r)[attn_q8_shape<D>::NPIECE], uint32_t & edge, const char * ring, int c0, int c1) {
    typedef attn_q8_shape<D> S;
    const int tid = threadIdx.x;
    const char * g0 = ring + (int64_t) c0 * S::ROWB;
    const int n = (c1 - c0) * S::ROWB;
    int pre = (int) ((16 - ((uintptr_t) g0 & 15)) & 15);
    pre = pre < n ? pre : n;
    const int nbody = (n - pre) / 16, tail = n - pre - nbody * 16;
    edge = 0;
    if (tid < 3 && tid * 4 < pre) edge = *(const uint32_t *) (g0 + tid * 4);
    if (tid >= 64 && tid < 67 && (tid - 64) * 4 < tail) edge = *(const uint32_t *) (g0 + pre + nbody * 16 + (tid - 64) * 4);
#pragma unroll
    for (int i = 0; i < S::NPIECE; i++) {   // (a range is one row at least: 68 bytes, so nbody >= 3)
        const int p = tid + i * ATTN_Q8_THREADS;
        r[i] = *(const attn_q8_u32x4 *) (g0 + pre + (p < nbody ? p : nbody - 1) * 16);
    }
}
// ... and put them into `buf` at the tile's own alignment modulo 16: slot c of the tile starts at byte ((uintptr_t) g0 & 15) + (c - c0) * ROWB
template <int D> __device__ __forceinline__ void attn_q8_store(const attn_q8_u32x4 (&r)[attn_q8_shape<D>::NPIECE], uint32_t edge, char * buf, const char * ring, int c0, int c1) {
    typedef attn_q8_shape<D> S;
    const int tid = threadIdx.x;
    const char * g0 = ring + (int64_t) c0 * S::ROWB;
    const int off0 = (int) ((uintptr_t) g0 & 15);
    const int n = (c1 - c0) * S::ROWB;
    int pre = (16 - off0) & 15;
    pre = pre < n ? pre : n;
    const int nbody = (n - pre) / 16, tail = n - pre - nbody * 16;
    if (tid < 3 && tid * 4 < pre) *(uint32_t *) (buf + off0 + tid * 4) = edge;
    if (tid >= 64 && tid < 67 && (tid - 64) * 4 < tail) *(uint32_t *) (buf + off0 + pre + nbody * 16 + (tid - 64) * 4) = edge;
#pragma unroll
    for (int i = 0; i < S::NPIECE; i++) {
        const int p = tid + i * ATTN_Q8_THREADS;
        if (p < nbody) *(attn_q8_u32x4 *) (buf + off0 + pre + p * 16) = r[i];
    }
}

template <int CTRL> __device__ __forceinline__ float attn_q8_quad(float v) { return dpp_f32<CTRL>(v); }

// A lane's four consecutive outputs of one head row, eight neighbouring lanes holding a block of 32 (every lane of the wave runs this: the block maximum
// travels by DPP). rotate: apply_rope's rotation of the pairs (in0, in1) by (rc, rs), `upper` for the outputs of the row's second half; otherwise in0 is
// the row. Then quantize_block_q80's arithmetic. -> the four quants, packed; dh: the block's scale as F16
__device__ __forceinline__ uint32_t attn_q8_rope_quant(const float (&in0)[4], const float (&in1)[4], const float (&rc)[4], const float (&rs)[4], bool rotate, bool upper, uint16_t & dh) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (rotate) {
            const float x0 = in0[i] * rc[i], x1 = in1[i] * rs[i], y0 = in0[i] * rs[i], y1 = in1[i] * rc[i];
            v[i] = upper ? y0 + y1 : x0 - x1;
        } else v[i] = in0[i];
    }
    float amax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
    amax = fmaxf(amax, dpp_f32<DPP_QUAD_XOR1>(amax));
    amax = fmaxf(amax, dpp_f32<DPP_QUAD_XOR2>(amax));
    amax = fmaxf(amax, dpp_f32<DPP_HALF_MIRROR>(amax));                 // the 8 lanes of one 32-wide block
    const float d = amax / 127.f;
    const float id = d != 0.f ? 1.0f / d : 0.0f;
    int q[4];
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = (int) roundf(v[i] * id);
    dh = f2h(d);
    return (uint32_t) (q[0] & 0xff) | ((uint32_t) (q[1] & 0xff) << 8) | ((uint32_t) (q[2] & 0xff) << 16) | ((uint32_t) (q[3] & 0xff) << 24);
}

template <int D>
__global__ void __launch_bounds__(ATTN_Q8_THREADS) attn_streams_q8_kernel(attn_streams_args sa) {
    typedef attn_q8_shape<D> S;
    constexpr int NBLK = S::NBLK, ROWB = S::ROWB, TILE = ATTN_Q8_TILE, half = D / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float sh_f[4];
    __shared__ double sh_d[4];
    __shared__ int sh_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x;
    const int64_t b = blockIdx.y;
    const attn_args & a = sa.a;
    const int C = a.C;

    float * sc = (float *) smem;                                            // [C] mask row -> scores -> exponentials -> probabilities
    char * p_ = smem + (((size_t) C * 4 + 15) & ~(size_t) 15);
    int8_t * qq = (int8_t *) p_; p_ += D;                                   // the quantised query ...
    float * qd = (float *) p_; p_ += 16;                                    // ... and its block scales (h2f of the F16 scale)
    char * knew = p_; p_ += S::ROW_Q8_BUF;                                     // the new K / V rows in ggml's row format
    char * vnew = p_; p_ += S::ROW_Q8_BUF;
    char * const buf0 = p_;                                                 // the two tile buffers, 16-byte aligned
    auto buf_of = [&](int t) { return buf0 + (t & 1) * S::BUF_Q8_BYTES; };
    double * red = (double *) p_;                                           // [G][D] partial outputs, once the last V tile has been consumed

    const float * mask = a.mask + b * sa.mask_bs;
    const char * kring = a.kcache + b * sa.kc_bs + (int64_t) h * a.k_nb2;
    const char * vring = a.vcache + b * sa.vc_bs + (int64_t) h * a.v_nb2;
    float * out = a.out + b * sa.out_bs + (int64_t) h * D;

    // ---- head: every load that waits for nothing ---------------------------------------------------------------------------------------------
    const int slot = a.index[b * sa.index_bs];
    float in0[4], in1[4], rc[4], rs[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { in0[i] = 0.f; in1[i] = 0.f; rc[i] = 1.f; rs[i] = 0.f; }
    const bool row_lane = wave < 3 && lane < D / 4;                        // wave 0: q, 1: k, 2: v; lane: outputs 4 lane .. 4 lane + 3
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
    constexpr int NMASK = ATTN_Q8_MAX_C / ATTN_Q8_THREADS;
    float mpre[NMASK];
#pragma unroll
    for (int i = 0; i < NMASK; i++) { const int c = tid + i * ATTN_Q8_THREADS; mpre[i] = mask[c < C ? c : C - 1]; }
    attn_q8_u32x4 regs[S::NPIECE];   // a tile's pieces between their request and their store to LDS
    uint32_t edge;
    const int c1_first = C < TILE ? C : TILE;                              // (valid memory whatever the mask says; slots beyond the live range are never looked at)
    attn_q8_request<D>(regs, edge, kring, 0, c1_first);

    // ---- RoPE and the three quantisers -----------------------------------------------------------------------------------------------------------
    if (wave < 3) {
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
    // ---- the live range: the mask row goes to the score buffer, its last un-masked slot ends the range -------------------------------------------
    int last = -1;
#pragma unroll
    for (int i = 0; i < NMASK; i++) {
        const int c = tid + i * ATTN_Q8_THREADS;
        if (c < C) { sc[c] = mpre[i]; if (mpre[i] > -INFINITY) last = c; }  // (ascending c: the last hit is the largest)
    }
    last = wave_allmax_i32(last);
    if (lane == 0) sh_i[wave] = last;
    attn_q8_store<D>(regs, edge, buf0, kring, 0, c1_first);
    __syncthreads();
    const int n_end = max(max(sh_i[0], sh_i[1]), max(sh_i[2], sh_i[3])) + 1;

    // the new rows go to their ring slot from LDS, packed
    if (slot >= 0 && slot < C) {
        if (D == 128) {
            if (tid < ROWB / 8) *(uint2 *) (const_cast<char *>(kring) + (int64_t) slot * a.k_nb1 + tid * 8) = *(const uint2 *) (knew + tid * 8);
            else if (tid >= 64 && tid < 64 + ROWB / 8) *(uint2 *) (const_cast<char *>(vring) + (int64_t) slot * a.v_nb1 + (tid - 64) * 8) = *(const uint2 *) (vnew + (tid - 64) * 8);
        } else {
            if (tid < ROWB / 4) *(uint32_t *) (const_cast<char *>(kring) + (int64_t) slot * a.k_nb1 + tid * 4) = *(const uint32_t *) (knew + tid * 4);
            else if (tid >= 64 && tid < 64 + ROWB / 4) *(uint32_t *) (const_cast<char *>(vring) + (int64_t) slot * a.v_nb1 + (tid - 64) * 4) = *(const uint32_t *) (vnew + (tid - 64) * 4);
        }
    }
    if (n_end <= 0) {   // a closed or empty column: zeros, as the BF16 body writes
        if (tid < D) out[tid] = 0.f;
        return;
    }
    const int NT = (n_end + TILE - 1) / TILE;
    auto tile_end = [&](int t) { const int e = (t + 1) * TILE; return e < n_end ? e : n_end; };
    // byte offset in a tile buffer (or, for the slot written this step, in the new row's buffer) of slot c of tile t - as an offset from smem
    auto slot_offset = [&](const char * ring, const char * fresh, int t, int c) {
        const int off0 = (int) ((uintptr_t) (ring + (int64_t) t * TILE * ROWB) & 15);
        return c == slot ? (int) (fresh - smem) : (int) (buf_of(t) - smem) + off0 + (c - t * TILE) * ROWB;
    };

    // ---- scores ----------------------------------------------------------------------------------------------------------------------------------
    {
        constexpr int LPS = NBLK, SPP = ATTN_Q8_THREADS / LPS;            // lanes per slot, slots per pass
        const int blk = tid % LPS, sp = tid / LPS;
        int qreg[8];
#pragma unroll
        for (int i = 0; i < 8; i++) qreg[i] = ((const int *) (qq + blk * 32))[i];
        const float dq = qd[blk];
        for (int t = 0; t < NT; t++) {
            // (tile 0 was requested for min(TILE, C) slots at entry: its first tile_end(0) slots are the ones looked at)
            if (t + 1 < NT) attn_q8_request<D>(regs, edge, kring, (t + 1) * TILE, tile_end(t + 1));
            const int c_hi = tile_end(t);
#pragma unroll
            for (int pass = 0; pass < TILE / SPP; pass++) {
                const int c = t * TILE + pass * SPP + sp, cc = c < c_hi ? c : c_hi - 1;
                const int A = slot_offset(kring, knew, t, cc) + blk * 34;   // the block: even, not always a dword boundary
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
                if (c < c_hi && blk == 0) {
                    const float m = sc[c];
                    float sv = -INFINITY;
                    if (m > -INFINITY) { sv = sumf * a.scale; sv = sv + m; }
                    sc[c] = sv;
                }
            }
            if (t + 1 < NT) attn_q8_store<D>(regs, edge, buf_of(t + 1), kring, (t + 1) * TILE, tile_end(t + 1));
            __syncthreads();
        }
    }
    // the first V tile is on its way during the soft_max
    attn_q8_request<D>(regs, edge, vring, 0, tile_end(0));

    // ---- soft_max --------------------------------------------------------------------------------------------------------------------------------
    float lmax = -INFINITY;
    for (int c = tid; c < n_end; c += ATTN_Q8_THREADS) lmax = fmaxf(lmax, sc[c]);
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
    attn_q8_store<D>(regs, edge, buf0, vring, 0, tile_end(0));
    __syncthreads();

    // ---- P x V -----------------------------------------------------------------------------------------------------------------------------------
    constexpr int LC = S::LC, G = S::G;
    const int lc = tid % LC, g = tid / LC;
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = 0;
    for (int t = 0; t < NT; t++) {
        if (t + 1 < NT) attn_q8_request<D>(regs, edge, vring, (t + 1) * TILE, tile_end(t + 1));
        const int c_hi = tile_end(t);
        for (int c = t * TILE + g; c < c_hi; c += G) {
            const float p = sc[c];
            const int A = slot_offset(vring, vnew, t, c) + (lc >> 2) * 34;   // the block of dims 8 lc ..
            const int Q = A + 2 + (lc & 3) * 8;                              // .. and their eight quants
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
        if (t + 1 < NT) attn_q8_store<D>(regs, edge, buf_of(t + 1), vring, (t + 1) * TILE, tile_end(t + 1));
        __syncthreads();
    }
    // (the barrier above: every tile has been consumed, the partial rows may lie over the buffers)
#pragma unroll
    for (int i = 0; i < 8; i++) red[g * D + lc * 8 + i] = acc[i];
    __syncthreads();
    if (tid < D) {
        double tot = 0;
        for (int gg = 0; gg < G; gg++) tot += red[gg * D + tid];            // fixed order: slot groups in index order
        out[tid] = (float) tot;
    }
}

bool k_attn_streams_q8_supported(const attn_streams_args & sa) {
    const attn_args & a = sa.a;
    const int64_t rowb = a.D / 32 * 34, al = a.D == 128 ? 8 : 4;           // (the packed ring stores: 8 bytes at D = 128, 4 at D = 64)
    if (sa.B < 2 || a.T != 1 || (a.D != 64 && a.D != 128) || a.C < 1 || a.C > ATTN_Q8_MAX_C || a.k_nb1 != rowb || a.v_nb1 != rowb) return false;
    for (int64_t v : { a.k_nb2, a.v_nb2, sa.kc_bs, sa.vc_bs, (int64_t) (uintptr_t) a.kcache, (int64_t) (uintptr_t) a.vcache }) if (v % al != 0) return false;
    return true;
}
void k_attn_streams_q8(hipStream_t s, const attn_streams_args & sa) {
    const attn_args & a = sa.a;
    GGML_ASSERT(k_attn_streams_q8_supported(sa));
    const size_t smem = a.D == 128 ? attn_q8_smem<128>(a.C) : attn_q8_smem<64>(a.C);
    GGML_ASSERT(smem <= 64 * 1024);                                        // (C <= 4096: 51.7 KB at D = 128 - no opt-in to larger LDS is needed)
    const dim3 grid((unsigned) a.H, (unsigned) sa.B);
    if (a.D == 128) attn_streams_q8_kernel<128><<<grid, ATTN_Q8_THREADS, smem, s>>>(sa);
    else            attn_streams_q8_kernel<64><<<grid, ATTN_Q8_THREADS, smem, s>>>(sa);
}
