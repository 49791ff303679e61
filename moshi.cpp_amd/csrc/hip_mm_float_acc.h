// Float-accumulating batched mat-mul for BF16 / F16 weights (T = 2..64 activation rows), included from hip_kernels_fused.hip after hip_mm_float.h.
// Opt-in (ggml_backend_mi355x_set_float_accumulate, MI355X_MMF=2): the f64 kernel of hip_mm_float.h stays the default.
//
// Numerics: the activation rows are rounded to the weight's type by the row converters of hip_mm_float.h, unchanged (same workspace, same bits as the
// f64 path and the oracle). A product of two BF16 / F16 values is exact in float; the SUMS are taken in float - inside v_mfma_f32_16x16x32_bf16 / _f16
// (32 k per instruction) and between the four waves' partial sums. Not bit-comparable with the oracle's double sum; bit-reproducible and
// column-independent (below).
//
// Operands of one MFMA (A[i][k] from lane (i = l & 15, k = 8 (l >> 4) .. + 7), B[k][j] from lane (k = 8 (l >> 4) .. + 7, j = l & 15)): the activation
// columns take the A side, the weight rows the B side - the one 16-byte load per operand that mm_f_mfma_kernel makes feeds one instruction for the whole
// 32-k chunk. Lane l = (r = l & 15, g = l >> 4) receives D[column 4 g + q][row r], q = 0..3 (the f32 16x16 result layout; the f64 one is g + 4 q).
//
// A column's result depends on K and its own values only - not on T, NT, M or its neighbours: the chunk -> wave deal (groups of MMA_U chunks
// round-robin) and the order of a wave's chunks are functions of K, the MFMA computes every D element from its own row / column, the waves' partial sums
// meet in LDS as ((w0 + w1) + w2) + w3. No atomics.
#pragma once

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

template <int WT>
__device__ __forceinline__ f32x4_t mma_step(const u32x4 x, const u32x4 w, const f32x4_t acc) {
    if constexpr (WT == GGML_TYPE_F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, x), __builtin_bit_cast(f16x8_t, w), acc, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, x), __builtin_bit_cast(bf16x8_t, w), acc, 0, 0, 0);
}

// A workgroup of four waves owns ONE 16-row tile, as in mm_f_mfma_kernel; the chunks are dealt in groups of MMA_U round-robin to the waves (wave w:
// chunks 4 w .. 4 w + 3, 4 w + 16 .., ..), each wave walks its chunks in increasing order with the next group requested before the current one is
// multiplied. One f32 MFMA per chunk and column tile leaves the matrix pipe idle most of the time: the group of four (4 KB of weights per wave in
// flight, 16 KB per workgroup) is what keeps the weight stream busy where two chunks did behind sixteen f64 instructions. Activations come straight
// from the workspace (L2).
#define MMA_U 4
template <int WT, int NT>
__global__ void __launch_bounds__(256) mm_f32acc_mfma_kernel(const char * w, int64_t row_bytes, int nch, int M, int T, const uint16_t * xa,
                                                             float * y, int64_t y_cs, const float * residual, int64_t r_cs) {
    __shared__ float red[3][NT * 4][64];
    // The wave index in a scalar register: every guard around an MFMA below is then a scalar branch. MFMA ignores EXEC, and a guard on a vector
    // condition is lowered to an EXEC mask WITHOUT a branch where the guarded block is short (one instruction here, sixteen in mm_f_mfma_kernel) -
    // the clamped copies of a ragged last group would be multiplied.
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * 16;
    const char * wp = w + (int64_t) (row0 + r < M ? row0 + r : M - 1) * row_bytes + g * 16;   // M tail: the last row again (not stored)
    const char * xp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) xp[nt] = (const char *) xa + (int64_t) (nt * 16 + r < T ? nt * 16 + r : T - 1) * nch * 64 + g * 16;
    f32x4_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) acc[nt] = f32x4_t{ 0, 0, 0, 0 };
    u32x4 wn[MMA_U], xn[MMA_U][NT];
    auto load = [&](int c0) {
#pragma unroll
        for (int u = 0; u < MMA_U; u++) {
            const int c = c0 + u < nch ? c0 + u : nch - 1;   // ragged last group: stay inside the row (the copy is not multiplied)
            wn[u] = __builtin_nontemporal_load((const u32x4 *) (wp + (int64_t) c * 64));
#pragma unroll
            for (int nt = 0; nt < NT; nt++) xn[u][nt] = *(const u32x4 *) (xp[nt] + (int64_t) c * 64);
        }
    };
    if (wave * MMA_U < nch) load(wave * MMA_U);
    for (int c0 = wave * MMA_U; c0 < nch; c0 += 4 * MMA_U) {
        u32x4 wc[MMA_U], xc[MMA_U][NT];
#pragma unroll
        for (int u = 0; u < MMA_U; u++) {
            wc[u] = wn[u];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) xc[u][nt] = xn[u][nt];
        }
        if (c0 + 4 * MMA_U < nch) load(c0 + 4 * MMA_U);
#pragma unroll
        for (int u = 0; u < MMA_U; u++)
            if (c0 + u < nch) {
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[nt] = mma_step<WT>(xc[u][nt], wc[u], acc[nt]);
            }
    }
    if (wave > 0) {
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int q = 0; q < 4; q++) red[wave - 1][nt * 4 + q][lane] = acc[nt][q];
    }
    __syncthreads();
    if (wave > 0) return;
    const int row = row0 + r;
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float v = acc[nt][q];
#pragma unroll
            for (int ww = 0; ww < 3; ww++) v += red[ww][nt * 4 + q][lane];
            const int col = nt * 16 + 4 * g + q;
            if (col >= T || row >= M) continue;
            if (residual) v = residual[(int64_t) col * r_cs + row] + v;
            y[(int64_t) col * y_cs + row] = v;
        }
}
