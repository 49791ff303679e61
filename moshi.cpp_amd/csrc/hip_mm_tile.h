// The float MFMA batched mat-muls, included from hip_kernels_fused.hip: ONE chunk-walk kernel, mm_mfma_kernel<Op, NT>, and the three operand
// structs that make its forms. A chunk is 32 k of one weight row / activation column; lane l = (r = l & 15, g = l >> 4) holds the 8 consecutive
// values at k = 8 g .. 8 g + 7 of weight row r and of activation column r of each of the NT column tiles. The activation columns take the A side of
// the MFMA, the weight rows the B side, so sixteen neighbouring lanes store sixteen neighbouring floats of one output column.
//
//   mm_op_f64<WT>     BF16 / F16 weights against rows rounded to the weight's type (hip_mm_cvt_rows.h), T = 2..64; the default. What ggml's generic
//                     product does (oracle.cpp vec_dot_bf16 / vec_dot_f16): every product exact, the sum kept in double, ONE rounding to float.
//                     v_mfma_f64_16x16x4_f64 keeps that form on the matrix pipe - BF16 / F16 widen to double exactly, a product of two 11-bit
//                     significands is exact in double. Only the ORDER of the double adds differs from the oracle's, ~2^-30 below the float rounding.
//   mm_op_f32acc<WT>  the same operands and workspace, opt-in (ggml_backend_mi355x_set_float_accumulate, MI355X_MMF=2): one v_mfma_f32_16x16x32_bf16
//                     / _f16 per chunk and column tile. A product of two BF16 / F16 values is exact in float; the SUMS are taken in float, inside
//                     the instruction and between the waves. Not bit-comparable with the oracle's double sum; bit-reproducible. DESIGN.md 24.
//   mm_op_f64_f32     F32 weights against the F32 activations as they are (no converter pass, no workspace), T = 2..128, opt-in
//                     (ggml_backend_mi355x_set_f32_matrix, MI355X_MMF32=1). Two floats widen to double exactly and their product is exact in double
//                     (24 + 24 significand bits fit in 53); a double sum, ONE rounding to float. The generic product and the oracle's vec_dot_f32
//                     round every product to float first, which a matrix instruction cannot do: nearer to the real product than theirs and NOT
//                     bit-comparable with them. DESIGN.md 31. (Its float work is loads, widenings and one add per output: there is no FP32
//                     arithmetic for the compiler to pair into packed instructions, and the ISA of the four instantiations holds none.)
//
// The two result lane maps: a 16x16x4 f64 step takes A[i][k] from lane (i = l & 15, k = l >> 4) and B[k][j] from lane (k = l >> 4, j = l & 15) - step
// j = 0..7 of a chunk feeds value j of both fragments, i.e. the four k's 8 g' + j - and leaves D[column g + 4 q][row r], q = 0..3, in lane l. The
// 16x16x32 f32 instruction takes k = 8 (l >> 4) .. + 7 from lane l, the whole fragment at once, and leaves D[column 4 g + q][row r]. Op::col is that map.
#pragma once

typedef double f64x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

template <int WT> __device__ __forceinline__ double mmf_lo(uint32_t u) { return (double) (WT == GGML_TYPE_F16 ? h2f((uint16_t) (u & 0xffff)) : __uint_as_float(u << 16)); }
template <int WT> __device__ __forceinline__ double mmf_hi(uint32_t u) { return (double) (WT == GGML_TYPE_F16 ? h2f((uint16_t) (u >> 16)) : __uint_as_float(u & 0xffff0000u)); }

// ---- what an Op gives: frag (a lane's 8 values of one chunk) and its load (weights non-temporal, activations plain), CHUNK_BYTES (32 k of a row),
// U (chunks per deal), acc_t (the accumulator of one column tile), chunk (multiply one chunk into every column tile) and col (the result lane map) ----
struct mm_frag16 {   // 8 BF16 / F16 values: one 16-byte load
    typedef u32x4 frag;
    static constexpr int CHUNK_BYTES = 64;
    template <bool WEIGHT> static __device__ __forceinline__ frag load(const char * p) { return WEIGHT ? __builtin_nontemporal_load((const u32x4 *) p) : *(const u32x4 *) p; }
};
template <int WT> struct mm_op_f64 : mm_frag16 {
    typedef f64x4_t acc_t;
    static constexpr int U = 2;
    template <int NT> static __device__ __forceinline__ void chunk(const frag (&xv)[NT], const frag wv, acc_t (&acc)[NT]) {   // 8 MFMA steps per column tile
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
    static __device__ __forceinline__ int col(int g, int q) { return g + 4 * q; }
};
// One f32 MFMA per chunk and column tile leaves the matrix pipe idle most of the time: the group of FOUR chunks (4 KB of weights per wave in flight,
// 16 KB per workgroup) is what keeps the weight stream busy where two chunks do behind the sixteen f64 instructions of the other forms.
template <int WT> struct mm_op_f32acc : mm_frag16 {
    typedef f32x4_t acc_t;
    static constexpr int U = 4;
    template <int NT> static __device__ __forceinline__ void chunk(const frag (&xv)[NT], const frag wv, acc_t (&acc)[NT]) {
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            if constexpr (WT == GGML_TYPE_F16) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, xv[nt]), __builtin_bit_cast(f16x8_t, wv), acc[nt], 0, 0, 0);
            else acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, xv[nt]), __builtin_bit_cast(bf16x8_t, wv), acc[nt], 0, 0, 0);
        }
    }
    static __device__ __forceinline__ int col(int g, int q) { return 4 * g + q; }
};
struct mm_op_f64_f32 {
    struct frag { f32x4_t h[2]; };   // 8 floats: two 16-byte loads
    typedef f64x4_t acc_t;
    static constexpr int CHUNK_BYTES = 128, U = 2;
    template <bool WEIGHT> static __device__ __forceinline__ frag load(const char * p) {
        const f32x4_t * v = (const f32x4_t *) p;
        return WEIGHT ? frag{ { __builtin_nontemporal_load(v), __builtin_nontemporal_load(v + 1) } } : frag{ { v[0], v[1] } };
    }
    template <int NT> static __device__ __forceinline__ void chunk(const frag (&xv)[NT], const frag wv, acc_t (&acc)[NT]) {   // 8 MFMA steps per column tile
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const double wd = (double) wv.h[j >> 2][j & 3];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64((double) xv[nt].h[j >> 2][j & 3], wd, acc[nt], 0, 0, 0);
        }
    }
    static __device__ __forceinline__ int col(int g, int q) { return g + 4 * q; }
};

// A workgroup of four waves owns ONE 16-row tile and at most four column tiles, columns blockIdx.y * 64 onwards (grid.y = 2 is the F32 form's T > 64:
// each half reads its weight tile through L2). The chunks are dealt in groups of U round-robin to the waves (wave v: chunks U v .. U v + U - 1,
// U v + 4 U .., ..); each wave walks its groups in increasing order, the next group requested before the current one is multiplied; the partial sums
// meet in LDS in the accumulator's type as ((w0 + w1) + w2) + w3. No atomics. Activations come straight from L2 (the workspace, or the <= 64 columns
// every workgroup re-reads): M / 16 reads of them per launch.
//
// A COLUMN'S RESULT DEPENDS ON K AND ITS OWN VALUES ONLY - not on T, NT, M, its grid.y half, its index or its neighbours: the chunk -> wave deal and
// the order of a wave's chunks are functions of K, the MFMA computes every D element from its own row / column, and the cross-wave order is fixed.
// Every B-column feature rests on this.
//
// (A second form for M >= 8192 - four waves owning 64 rows, walking K together over an activation step staged once in LDS - measured 9 / 15 / 13 %
// slower per step at B = 16 / 32 / 64 and was removed: the kernel is bound by the f64 matrix pipe, not by the activation reads, and the form's two
// barriers per step idle that pipe. DESIGN.md 23.)
//
// w: row stride row_bytes (16-byte aligned, >= nch chunks); x: column stride x_cb BYTES (nch * 64 for the workspace, 4 x_cs for F32 activations;
// x and x_cb 16-byte aligned). Rows past M and columns past T read the last valid one (the copies are multiplied, never stored).
template <typename Op, int NT>
__global__ void __launch_bounds__(256) mm_mfma_kernel(const char * w, int64_t row_bytes, int nch, int M, int T, const char * x, int64_t x_cb,
                                                      float * y, int64_t y_cs, const float * residual, int64_t r_cs) {
    typedef typename Op::frag frag;
    typedef typename Op::acc_t acc_t;
    typedef decltype(acc_t{}[0] + 0) sum_t;
    constexpr int U = Op::U, CB = Op::CHUNK_BYTES;
    __shared__ sum_t red[3][NT * 4][64];
    // The wave index in a scalar register: every guard around an MFMA below is then a scalar branch. MFMA ignores EXEC, and a guard on a vector
    // condition is lowered to an EXEC mask WITHOUT a branch where the guarded block is short (one instruction in mm_op_f32acc) - the clamped copies
    // of a ragged last group would be multiplied.
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * 16, col0 = blockIdx.y * 64;
    T -= col0;                                    // this half's columns: 0 .. T - 1 of x, y and residual moved to col0
    x += (int64_t) col0 * x_cb; y += (int64_t) col0 * y_cs;
    if (residual) residual += (int64_t) col0 * r_cs;
    const char * wp = w + (int64_t) (row0 + r < M ? row0 + r : M - 1) * row_bytes + g * (CB / 4);
    const char * xp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) xp[nt] = x + (int64_t) (nt * 16 + r < T ? nt * 16 + r : T - 1) * x_cb + g * (CB / 4);
    acc_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) acc[nt] = acc_t{ 0, 0, 0, 0 };
    frag wn[U], xn[U][NT];
    auto load = [&](int c0) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int c = c0 + u < nch ? c0 + u : nch - 1;   // ragged last group: stay inside the row (the copy is not multiplied)
            wn[u] = Op::template load<true>(wp + (int64_t) c * CB);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) xn[u][nt] = Op::template load<false>(xp[nt] + (int64_t) c * CB);
        }
    };
    if (wave * U < nch) load(wave * U);
    for (int c0 = wave * U; c0 < nch; c0 += 4 * U) {
        frag wc[U], xc[U][NT];
#pragma unroll
        for (int u = 0; u < U; u++) {
            wc[u] = wn[u];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) xc[u][nt] = xn[u][nt];
        }
        if (c0 + 4 * U < nch) load(c0 + 4 * U);
#pragma unroll
        for (int u = 0; u < U; u++) if (c0 + u < nch) Op::chunk(xc[u], wc[u], acc);
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
            sum_t sum = acc[nt][q];
#pragma unroll
            for (int ww = 0; ww < 3; ww++) sum += red[ww][nt * 4 + q][lane];
            const int col = nt * 16 + Op::col(g, q);
            if (col >= T || row >= M) continue;
            float v = (float) sum;
            if (residual) v = residual[(int64_t) col * r_cs + row] + v;
            y[(int64_t) col * y_cs + row] = v;
        }
}
