// A codec convolution group at B columns (decoder / encoder slots) as ONE launch of F16 MFMA tiles, included from hip_kernels_generic.hip behind
// k_conv_cols. Opt-in (bit 2 of ggml_backend_mi355x_set_f32_matrix, MI355X_MMF32=4..7): the elu / concat / cpy / im2col / k_conv_cols / add launches
// stay the default. An implicit-im2col GEMM: neither the concat nor the im2col tensor exists.
//
//   x [Lx, IC, B] F32 through element strides xs0 / xs1 / xs2 (ELU in front when pre_elu), prev [TP, IC, B] F32 dense (TP = 0: a stateless convolution), w [Kw, IC, OC] F16 dense,
//   xcat[b][ic] = concat(prev[b][ic][0..TP), act(x[b][ic][0..Lx))),  OW = (TP + Lx - Kw) / s0 + 1 positions per column,  K = IC Kw.
//   position p = b OW + ow, k = ic Kw + tap:  A[p][k] = f16(xcat[b][ic][ow s0 + tap]);  W[oc][k] = w as stored
//   out[ow, oc, b] = resid[ow, oc, b] + ((sum over k of A[p][k] W[oc][k]) + bias[oc]);  prev[b][ic][j] = xcat[b][ic][Lx + j]
//
// Numerics: the activation is rounded to F16 as ggml_im2col does, every product of two F16 values is exact in float, and an output is
// ONE float accumulator over the whole of K in ascending chunks of 32 (v_mfma_f32_16x16x32_f16). K is split neither across waves nor across
// workgroups, a chunk past K is zero on both sides, so a column's bits depend on the layer and the column's own values only - which lane, tile or
// workgroup holds an output depends on B, its value does not. NOT k_conv_cols' bits (double sums in its dot / short forms, SK float slices in its tile form).
//
// Split. A workgroup of four waves owns a RUN of 16 NT consecutive positions (NT = 1..4 position tiles; a run crosses column borders, the last one is
// ragged: rows past B OW are clamped on load and never stored) and a SLAB of `ts` 16-wide OC tiles (grid.y; ts halves from 8 until the grid holds
// CVM_TARGET_WGS workgroups). Wave v owns OC tiles v, v + 4 of the slab and keeps one f32x4 accumulator per (OC tile, position tile) for all of K.
//
// LDS. K is walked in slabs of CVM_KS = 128. All 256 threads build the slab's im2col rows from prev / x (ELU on the x part, F16 rounding): a thread
// makes 8 consecutive k of one position and stores them as one 16-byte word, consecutive threads take consecutive positions. Row pitch 136 halves
// (68 words): the 16 rows of a tile start 4 banks apart, so a lane's 16-byte read of (row r, k = 32 c + 8 g) meets no other row of its tile. Two
// buffers: slab s + 1 is staged, and its weight fragments requested, before slab s is multiplied; one barrier per slab.
//
// Registers. The weight fragment of lane (r = lane & 15, g = lane >> 4) for OC tile t and chunk c is row oc = 16 t + r, halves k = 32 c + 8 g .. + 7: one
// 16-byte non-temporal load where the rows are 16-byte aligned (K % 8 == 0), eight 2-byte loads otherwise (K = 7, 3 ...); halves past K are zero.
// A fragment meets every position tile of the run, so the weights stream once per 64 positions. The lane holds D[position 4 g + q][channel r], q = 0..3.
//
// Epilogue: + bias, then resid + that, stored as [OW, OC, B]; 16 bytes where the lane's four positions lie in one column at an aligned address.
//
// The carried tail: every workgroup reads prev (its columns' first positions), so prev is written by the LAST workgroup to arrive - the ticket of
// vq_level_cols_kernel: drawn behind the barrier that ends the K walk (every load of prev has returned by then), from a counter in the plan's
// workspace that the last arriver resets. It walks the B IC TP tail values in rounds of 256 x CVM_TAIL_U: read (a value that survives, TP > Lx,
// lies Lx elements AHEAD in prev - the same round or a later one), barrier, store. No workgroup waits for another.
#pragma once

#define CVM_KS 128          // k of a slab: four 32-chunks
#define CVM_PITCH 136       // halves of an LDS row
#define CVM_TW 2            // OC tiles of a wave
#define CVM_TARGET_WGS 256
#define CVM_TAIL_U 16

struct conv_mfma_args {
    const float * x; float * prev; const uint16_t * w; const float * bias; const float * resid; float * out; unsigned * counter;
    int64_t xs0, xs1, xs2;   // element strides of x
    int IC, OC, Kw, s0, Lx, TP, OW, B, ts, pre_elu;
};

// the 8 weight halves of row `row` at k0 .. k0 + 7 (zero past K)
__device__ __forceinline__ f16x8 cvm_load_w(const uint16_t * w, int64_t row, int k0, int K, bool vec) {
    f16x8 v = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (vec) { if (k0 < K) v = __builtin_nontemporal_load((const f16x8 *) (w + row * K + k0)); }
    else {
#pragma unroll
        for (int e = 0; e < 8; e++) if (k0 + e < K) { const uint16_t h = w[row * K + k0 + e]; _Float16 f; __builtin_memcpy(&f, &h, 2); v[e] = f; }
    }
    return v;
}

template <int NT>
__global__ void __launch_bounds__(256) conv_cols_implicit_mfma_kernel(conv_mfma_args a) {
    __shared__ __attribute__((aligned(16))) _Float16 As[2][NT * 16 * CVM_PITCH];
    __shared__ int s_last;
    constexpr int ROWS = NT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int K = a.IC * a.Kw, P = a.B * a.OW, Lx = a.Lx, TP = a.TP, Kw = a.Kw;
    const int run0 = blockIdx.x * ROWS;
    const int nslabs = (K + CVM_KS - 1) / CVM_KS, nchunks = (K + 31) / 32;
    const bool wvec = K % 8 == 0 && ((uintptr_t) a.w & 15) == 0;

    // staging units of this thread: unit u = tid + 256 j is (row u % ROWS, the 8 k at 8 (u / ROWS)) of a slab
    int st_i0[NT], st_b[NT];   // ow s0 and b of the unit's position
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int p = min(run0 + (tid + 256 * j) % ROWS, P - 1), b = p / a.OW;
        st_i0[j] = (p - b * a.OW) * a.s0; st_b[j] = b;
    }
    auto stage = [&](int slab, _Float16 * dst) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int u = tid + 256 * j, row = u % ROWS, k8 = u / ROWS;
            int k = slab * CVM_KS + k8 * 8, ic = k / Kw, tap = k - ic * Kw;
            f16x8 h;
#pragma unroll
            for (int e = 0; e < 8; e++, k++) {
                float v = 0.f;
                if (k < K) {
                    const int i = st_i0[j] + tap;
                    if (i < TP) v = a.prev[((int64_t) st_b[j] * a.IC + ic) * TP + i];
                    else { v = a.x[st_b[j] * a.xs2 + ic * a.xs1 + (i - TP) * a.xs0]; if (a.pre_elu) v = v > 0.f ? v : expm1f(v); }
                }
                h[e] = (_Float16) v;
                if (++tap == Kw) { tap = 0; ic++; }
            }
            *(f16x8 *) (dst + row * CVM_PITCH + k8 * 8) = h;
        }
    };

    // this wave's OC tiles
    const int tile0 = blockIdx.y * a.ts;
    bool live[CVM_TW]; int64_t wrow[CVM_TW];
#pragma unroll
    for (int t = 0; t < CVM_TW; t++) {
        const int tl = wave + 4 * t;
        live[t] = tl < a.ts && (tile0 + tl) * 16 < a.OC;
        wrow[t] = min((tile0 + tl) * 16 + r, a.OC - 1);
    }
    f16x8 wn[CVM_TW][4], wc[CVM_TW][4];
    auto load_w = [&](int slab) {
#pragma unroll
        for (int t = 0; t < CVM_TW; t++)
#pragma unroll
            for (int c = 0; c < 4; c++) wn[t][c] = live[t] ? cvm_load_w(a.w, wrow[t], slab * CVM_KS + 32 * c + 8 * g, K, wvec) : f16x8{ 0, 0, 0, 0, 0, 0, 0, 0 };
    };
    f32x4 acc[CVM_TW][NT];
#pragma unroll
    for (int t = 0; t < CVM_TW; t++)
#pragma unroll
        for (int pt = 0; pt < NT; pt++) acc[t][pt] = f32x4{ 0.f, 0.f, 0.f, 0.f };

    load_w(0);
    stage(0, As[0]);
    __syncthreads();
    for (int s = 0; s < nslabs; s++) {
#pragma unroll
        for (int t = 0; t < CVM_TW; t++)
#pragma unroll
            for (int c = 0; c < 4; c++) wc[t][c] = wn[t][c];
        if (s + 1 < nslabs) { load_w(s + 1); stage(s + 1, As[(s + 1) & 1]); }
        const _Float16 * ab = As[s & 1] + r * CVM_PITCH + g * 8;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (s * 4 + c < nchunks) {
                f16x8 av[NT];
#pragma unroll
                for (int pt = 0; pt < NT; pt++) av[pt] = *(const f16x8 *) (ab + pt * 16 * CVM_PITCH + c * 32);
#pragma unroll
                for (int t = 0; t < CVM_TW; t++) {
                    if (live[t]) {
#pragma unroll
                        for (int pt = 0; pt < NT; pt++) acc[t][pt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[pt], wc[t][c], acc[t][pt], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }

    // epilogue: lane (r, g) holds positions run0 + 16 pt + 4 g + q of channel 16 tile + r
    const bool out16 = ((uintptr_t) a.out & 15) == 0 && (!a.resid || ((uintptr_t) a.resid & 15) == 0);
#pragma unroll
    for (int t = 0; t < CVM_TW; t++) {
        const int oc = (tile0 + wave + 4 * t) * 16 + r;
        if (!live[t] || oc >= a.OC) continue;
        const float bv = a.bias ? a.bias[oc] : 0.f;
#pragma unroll
        for (int pt = 0; pt < NT; pt++) {
            const int p = run0 + 16 * pt + 4 * g;
            if (p >= P) continue;
            const int b = p / a.OW, ow = p - b * a.OW;
            const int64_t o = ((int64_t) b * a.OC + oc) * a.OW + ow;
            f32x4 v = acc[t][pt];
            if (ow + 3 < a.OW && (o & 3) == 0 && out16) {
                if (a.bias) { v[0] = v[0] + bv; v[1] = v[1] + bv; v[2] = v[2] + bv; v[3] = v[3] + bv; }
                if (a.resid) { const f32x4 x = *(const f32x4 *) (a.resid + o); v[0] = x[0] + v[0]; v[1] = x[1] + v[1]; v[2] = x[2] + v[2]; v[3] = x[3] + v[3]; }
                *(f32x4 *) (a.out + o) = v;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int pq = p + q;
                    if (pq >= P) break;
                    const int bq = pq / a.OW;
                    const int64_t oq = ((int64_t) bq * a.OC + oc) * a.OW + (pq - bq * a.OW);
                    float y = v[q];
                    if (a.bias) y = y + bv;
                    if (a.resid) y = a.resid[oq] + y;
                    a.out[oq] = y;
                }
            }
        }
    }

    // the carried tail, by the last workgroup to arrive
    if (TP == 0) return;
    if (tid == 0) s_last = atomicAdd(a.counter, 1u) == gridDim.x * gridDim.y - 1;
    __syncthreads();
    if (!s_last) return;
    const int64_t N = (int64_t) a.B * a.IC * TP;
    const bool survives = Lx < TP;
    for (int64_t base = 0; base < N; base += 256 * CVM_TAIL_U) {
        float v[CVM_TAIL_U];
#pragma unroll
        for (int u = 0; u < CVM_TAIL_U; u++) {
            const int64_t e = base + u * 256 + tid;
            if (e < N) {
                const int64_t row = e / TP; const int i = Lx + (int) (e - row * TP);
                if (i < TP) v[u] = a.prev[row * TP + i];
                else { const int64_t b = row / a.IC; v[u] = a.x[b * a.xs2 + (row - b * a.IC) * a.xs1 + (i - TP) * a.xs0]; if (a.pre_elu) v[u] = v[u] > 0.f ? v[u] : expm1f(v[u]); }
            }
        }
        if (survives) __syncthreads();
#pragma unroll
        for (int u = 0; u < CVM_TAIL_U; u++) {
            const int64_t e = base + u * 256 + tid;
            if (e < N) a.prev[e] = v[u];
        }
    }
    if (tid == 0) *a.counter = 0u;
}
