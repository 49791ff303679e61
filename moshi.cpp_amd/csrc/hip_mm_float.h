// Batched mat-mul for BF16 / F16 weights (T = 2..64 activation rows), included from hip_kernels_fused.hip.
//
// Numerics: what ggml's generic BF16 / F16 product does (oracle.cpp vec_dot_bf16 / vec_dot_f16) - activation rows rounded to the weight's type, every
// product exact, the sum kept in double, ONE rounding to float. v_mfma_f64_16x16x4_f64 keeps that form on the matrix pipe: BF16 / F16 values widen to
// double exactly, a product of two 11-bit significands is exact in double, the accumulators are double. Only the ORDER of the double adds differs
// from the oracle's, which sits ~2^-30 below the final float rounding.
//
// Operands of one MFMA step (A[i][k] from lane (i = l & 15, k = l >> 4), B[k][j] from lane (k = l >> 4, j = l & 15)): the activation columns take the
// A side, the weight rows the B side, so lane l = (r = l & 15, g = l >> 4) receives D[column g + 4 q][row r], q = 0..3 - sixteen neighbouring lanes
// store sixteen neighbouring floats of one output column. For a chunk of 32 k lane l loads the 8 consecutive values of weight row r at kb + 8 g and the
// same 8 of activation column r of each column tile (one 16-byte load each); step j = 0..7 feeds value j of both, i.e. the four k's kb + 8 g' + j.
//
// A column's result depends on K and its own values only - not on T, NT or its neighbours: the chunk -> wave deal and the order of the chunks are a
// function of K, the MFMA computes every D element from its own row / column, the waves are summed 1, 2, 3 onto 0.
#pragma once

typedef double f64x4_t __attribute__((ext_vector_type(4)));

template <int WT> __device__ __forceinline__ uint16_t mmf_round(float v) { return WT == GGML_TYPE_F16 ? f2h(v) : f2bf(v); }
template <int WT> __device__ __forceinline__ double mmf_lo(uint32_t u) { return (double) (WT == GGML_TYPE_F16 ? h2f((uint16_t) (u & 0xffff)) : __uint_as_float(u << 16)); }
template <int WT> __device__ __forceinline__ double mmf_hi(uint32_t u) { return (double) (WT == GGML_TYPE_F16 ? h2f((uint16_t) (u >> 16)) : __uint_as_float(u & 0xffff0000u)); }
template <int WT> __device__ __forceinline__ u32x4 mmf_pack8(const float v[8]) {
    u32x4 o;
    o.x = (uint32_t) mmf_round<WT>(v[0]) | ((uint32_t) mmf_round<WT>(v[1]) << 16); o.y = (uint32_t) mmf_round<WT>(v[2]) | ((uint32_t) mmf_round<WT>(v[3]) << 16);
    o.z = (uint32_t) mmf_round<WT>(v[4]) | ((uint32_t) mmf_round<WT>(v[5]) << 16); o.w = (uint32_t) mmf_round<WT>(v[6]) | ((uint32_t) mmf_round<WT>(v[7]) << 16);
    return o;
}

// ---- activation rows F32 -> the weight's type, dense [T][K] in the workspace (K % 8 == 0) ---------------------------------------------------
template <int WT>
__global__ void __launch_bounds__(256) cvt_rows_kernel(const float * x, int64_t x_cs, int K, int64_t total8, uint16_t * out) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= total8) return;
    const int k8 = K / 8;
    const int64_t t = i / k8; const int k = (int) (i - t * k8) * 8;
    const float4 a = *(const float4 *) (x + t * x_cs + k), b = *(const float4 *) (x + t * x_cs + k + 4);
    const float v[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
    *(u32x4 *) (out + t * K + k) = mmf_pack8<WT>(v);
}
// alpha * rms_norm(x): the statistics in double with matvec_f_kernel's partition (thread tid takes i = tid, tid + 256, ..; waves summed 0 + 1 + 2 + 3)
template <int WT>
__global__ void __launch_bounds__(256) rms_cvt_rows_kernel(const float * x, int64_t x_cs, const float * alpha, float eps, int K, uint16_t * out) {
    __shared__ double sh[4];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float * row = x + (int64_t) t * x_cs;
    double acc = 0;
    for (int i = tid; i < K; i += 256) { const float v = row[i]; acc += (double) (v * v); }
    acc = wave_allsum_f64(acc);
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    const float scale = 1.0f / sqrtf((float) ((sh[0] + sh[1] + sh[2] + sh[3]) / (double) K) + eps);
    for (int k = tid * 8; k < K; k += 2048) {
        const float4 x0 = *(const float4 *) (row + k), x1 = *(const float4 *) (row + k + 4), a0 = *(const float4 *) (alpha + k), a1 = *(const float4 *) (alpha + k + 4);
        const float v[8] = { a0.x * (x0.x * scale), a0.y * (x0.y * scale), a0.z * (x0.z * scale), a0.w * (x0.w * scale),
                             a1.x * (x1.x * scale), a1.y * (x1.y * scale), a1.z * (x1.z * scale), a1.w * (x1.w * scale) };
        *(u32x4 *) (out + (int64_t) t * K + k) = mmf_pack8<WT>(v);
    }
}
// silu(h[:K]) * h[K:]
template <int WT>
__global__ void __launch_bounds__(256) gate_cvt_rows_kernel(const float * h, int64_t h_cs, int K, int64_t total8, uint16_t * out) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= total8) return;
    const int k8 = K / 8;
    const int64_t t = i / k8; const int k = (int) (i - t * k8) * 8;
    const float * hl = h + t * h_cs + k;
    const float4 l0 = *(const float4 *) hl, l1 = *(const float4 *) (hl + 4), r0 = *(const float4 *) (hl + K), r1 = *(const float4 *) (hl + K + 4);
    const float l[8] = { l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w }, r[8] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w };
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = (l[j] / (1.0f + expf(-l[j]))) * r[j];
    *(u32x4 *) (out + t * K + k) = mmf_pack8<WT>(v);
}

// ---- the product --------------------------------------------------------------------------------------------------------------------------
// one chunk of 32 k: 8 MFMA steps per column tile
template <int WT, int NT>
__device__ __forceinline__ void mmf_chunk(const u32x4 wv, const u32x4 (&xv)[NT], f64x4_t (&acc)[NT]) {
    const uint32_t wu[4] = { wv.x, wv.y, wv.z, wv.w };
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double w0 = mmf_lo<WT>(wu[j]), w1 = mmf_hi<WT>(wu[j]);
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            const uint32_t xu = j == 0 ? xv[nt].x : j == 1 ? xv[nt].y : j == 2 ? xv[nt].z : xv[nt].w;
            acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(mmf_lo<WT>(xu), w0, acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(mmf_hi<WT>(xu), w1, acc[nt], 0, 0, 0);
        }
    }
}
template <int NT>
__device__ __forceinline__ void mmf_store(const f64x4_t (&acc)[NT], int row, int g, int M, int T, float * y, int64_t y_cs, const float * residual, int64_t r_cs) {
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int col = nt * 16 + g + 4 * q;
            if (col >= T || row >= M) continue;
            float v = (float) acc[nt][q];
            if (residual) v = residual[(int64_t) col * r_cs + row] + v;
            y[(int64_t) col * y_cs + row] = v;
        }
}

// A workgroup of four waves owns ONE 16-row tile; the chunks are dealt in pairs round-robin to the waves (wave w: chunks 2 w, 2 w + 1,
// 2 w + 8, ..), each wave walks its chunks in increasing order with the next pair requested before the current one is multiplied; partial sums meet in
// LDS in double, waves 1, 2, 3 onto wave 0. Activations come straight from the workspace (L2): M / 16 reads of it per launch. (A second form for
// M >= 8192 - four waves owning 64 rows, walking K together over an activation step staged once in LDS - measured 9 / 15 / 13 % slower per step at B = 16 / 32 / 64 and was
// removed: the kernel is bound by the f64 matrix pipe, not by the activation reads, and the form's two barriers per step idle that pipe. DESIGN.md 23.)
#define MMF_U 2
template <int WT, int NT>
__global__ void __launch_bounds__(256) mm_f_mfma_kernel(const char * w, int64_t row_bytes, int nch, int M, int T, const uint16_t * xa,
                                                        float * y, int64_t y_cs, const float * residual, int64_t r_cs) {
    __shared__ double red[3][NT * 4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * 16;
    const char * wp = w + (int64_t) (row0 + r < M ? row0 + r : M - 1) * row_bytes + g * 16;
    const char * xp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) xp[nt] = (const char *) xa + (int64_t) (nt * 16 + r < T ? nt * 16 + r : T - 1) * nch * 64 + g * 16;
    f64x4_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) acc[nt] = f64x4_t{ 0, 0, 0, 0 };
    u32x4 wn[MMF_U], xn[MMF_U][NT];
    auto load = [&](int c0) {
#pragma unroll
        for (int u = 0; u < MMF_U; u++) {
            const int c = c0 + u < nch ? c0 + u : nch - 1;   // ragged last pair: stay inside the row (the copy is not multiplied)
            wn[u] = __builtin_nontemporal_load((const u32x4 *) (wp + (int64_t) c * 64));
#pragma unroll
            for (int nt = 0; nt < NT; nt++) xn[u][nt] = *(const u32x4 *) (xp[nt] + (int64_t) c * 64);
        }
    };
    if (wave * MMF_U < nch) load(wave * MMF_U);
    for (int c0 = wave * MMF_U; c0 < nch; c0 += 4 * MMF_U) {
        u32x4 wc[MMF_U], xc[MMF_U][NT];
#pragma unroll
        for (int u = 0; u < MMF_U; u++) {
            wc[u] = wn[u];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) xc[u][nt] = xn[u][nt];
        }
        if (c0 + 4 * MMF_U < nch) load(c0 + 4 * MMF_U);
#pragma unroll
        for (int u = 0; u < MMF_U; u++) if (c0 + u < nch) mmf_chunk<WT, NT>(wc[u], xc[u], acc);
    }
    if (wave > 0) {
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int q = 0; q < 4; q++) red[wave - 1][nt * 4 + q][lane] = acc[nt][q];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int ww = 0; ww < 3; ww++) acc[nt][q] += red[ww][nt * 4 + q][lane];
    mmf_store<NT>(acc, row0 + r, g, M, T, y, y_cs, residual, r_cs);
}
