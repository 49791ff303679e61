// Batched mat-mul for F32 weights (T = 2..128 activation rows), included from hip_kernels_fused.hip after hip_mm_float.h (f64x4_t, mmf_store).
// Opt-in (ggml_backend_mi355x_set_f32_matrix, MI355X_MMF32=1): the generic product (mul_mat_kernel, a wave per output) stays the default.
//
// Numerics: two floats widen to double exactly, their product is exact in double (24 + 24 significand bits fit in 53), the sum is kept in double with
// ONE rounding to float. The generic product and the oracle's vec_dot_f32 round every product to float before they add it in double, which a matrix
// instruction cannot do: this form is nearer to the real product than theirs and NOT bit-comparable with them. DESIGN.md 31.
//
// Operands of one v_mfma_f64_16x16x4_f64 step: the lane map at the top of hip_mm_float.h - the activation columns take the A side, the weight rows
// the B side, lane l = (r = l & 15, g = l >> 4) receives D[column g + 4 q][row r], q = 0..3. For a chunk of 32 k lane l loads the 8 consecutive floats
// of weight row r at kb + 8 g (two 16-byte loads, non-temporal) and the same 8 of activation column r of each column tile; step j = 0..7 feeds value
// j of both through v_cvt_f64_f32, i.e. the four k's kb + 8 g' + j. There is no converter pass and no workspace: the activations are read as they
// are (every workgroup of a launch re-reads the same <= 64 columns, which stay in L2) and the launch is the whole product.
//
// A workgroup of four waves owns ONE 16-row tile and at most four column tiles; T > 64 is grid.y = 2 (columns 0..63 and 64..127, each half reading
// its weight tile through L2). The chunks are dealt in pairs round-robin to the waves (wave w: chunks 2 w, 2 w + 1, 2 w + 8, ..), each wave walks its
// chunks in increasing order with the next pair requested before the current one is multiplied; partial sums meet in LDS in double, waves 1, 2, 3
// onto wave 0.
//
// A column's result depends on K and its own values only - not on T, NT, its grid.y half, its index or its neighbours: the chunk -> wave deal and the
// order of the chunks are a function of K, the MFMA computes every D element from its own row / column, the waves are summed 1, 2, 3 onto 0.
#pragma once

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// one chunk of 32 k: 8 MFMA steps per column tile
template <int NT>
__device__ __forceinline__ void mm32_chunk(const f32x4_t (&wv)[2], const f32x4_t (&xv)[NT][2], f64x4_t (&acc)[NT]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const double wd = (double) wv[j >> 2][j & 3];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64((double) xv[nt][j >> 2][j & 3], wd, acc[nt], 0, 0, 0);
    }
}

// rows: w row stride row_bytes (16-byte aligned, >= 128 nch bytes); columns: x column stride x_cs floats (x and x_cs * 4 16-byte aligned). Rows past M
// and columns past T are clamped on load (the copies are multiplied, never stored).
// (The float work of this kernel is loads, widenings and one add per output: there is no FP32 arithmetic for the compiler to pair into packed
// instructions, and the ISA of the four instantiations holds none.)
#define MM32_U 2
template <int NT>
__global__ void __launch_bounds__(256) mm_f32_mfma_kernel(const char * w, int64_t row_bytes, int nch, int M, int T, const float * x, int64_t x_cs,
                                                          float * y, int64_t y_cs, const float * residual, int64_t r_cs) {
    __shared__ double red[3][NT * 4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * 16, col0 = blockIdx.y * 64;
    T -= col0;                                    // this half's columns: 0 .. T - 1 of x, y and residual moved to col0
    x += (int64_t) col0 * x_cs; y += (int64_t) col0 * y_cs;
    if (residual) residual += (int64_t) col0 * r_cs;
    const char * wp = w + (int64_t) (row0 + r < M ? row0 + r : M - 1) * row_bytes + g * 32;
    const char * xp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) xp[nt] = (const char *) (x + (int64_t) (nt * 16 + r < T ? nt * 16 + r : T - 1) * x_cs) + g * 32;
    f64x4_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) acc[nt] = f64x4_t{ 0, 0, 0, 0 };
    f32x4_t wn[MM32_U][2], xn[MM32_U][NT][2];
    auto load = [&](int c0) {
#pragma unroll
        for (int u = 0; u < MM32_U; u++) {
            const int c = c0 + u < nch ? c0 + u : nch - 1;   // ragged last pair: stay inside the row (the copy is not multiplied)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                wn[u][h] = __builtin_nontemporal_load((const f32x4_t *) (wp + (int64_t) c * 128 + h * 16));
#pragma unroll
                for (int nt = 0; nt < NT; nt++) xn[u][nt][h] = *(const f32x4_t *) (xp[nt] + (int64_t) c * 128 + h * 16);
            }
        }
    };
    if (wave * MM32_U < nch) load(wave * MM32_U);
    for (int c0 = wave * MM32_U; c0 < nch; c0 += 4 * MM32_U) {
        f32x4_t wc[MM32_U][2], xc[MM32_U][NT][2];
#pragma unroll
        for (int u = 0; u < MM32_U; u++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                wc[u][h] = wn[u][h];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) xc[u][nt][h] = xn[u][nt][h];
            }
        if (c0 + 4 * MM32_U < nch) load(c0 + 4 * MM32_U);
#pragma unroll
        for (int u = 0; u < MM32_U; u++) if (c0 + u < nch) mm32_chunk<NT>(wc[u], xc[u], acc);
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
