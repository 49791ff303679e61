// The streaming transposed convolution at B columns (decoder slots) as ONE launch of f64 MFMA tiles, included from hip_kernels_generic.hip next to
// k_convtr_cols. Opt-in (bit 1 of ggml_backend_mi355x_set_f32_matrix, MI355X_MMF32=2 / 3): the partial + finish pair stays the default.
//
//   x [L, IC, B] F32 dense (ELU in front when pre_elu), w [K, OC, IC] F32 dense with K == 2 s0, prev [(L + 1) s0, OC, B], out [L s0, OC, B].
//   n = oc K + k:  Z[p][n] = sum over ic of x[l, ic, b] w[ic][n]  at position p = b L + l;  z = (float) Z
//   t = l s0 + j:  y[t] = z[l - 1][oc, j + s0] + z[l][oc, j]  (l = 0: z[0][oc, j] + the old prev[L s0 + j]);  prev[t] = y[t];  out[t] = y[t] + bias[oc]
//                  prev[L s0 + j] = z[L - 1][oc, j + s0]
//
// Numerics: both operands widen to double exactly, every product is exact in double, ONE double accumulator per (p, n) runs over the
// whole of IC in ascending ic (four ic per v_mfma_f64_16x16x4_f64 step) and is rounded once to float; the two taps, the old tail and the bias are
// float adds. The partial + finish pair rounds every product to float first: nearer to the real value here, NOT bit-comparable with it.
//
// Split. A workgroup of four waves owns a CHANNEL GROUP - the lcm(K, 16) / K channels whose K taps fill whole 16-wide n tiles (NTG = 1, 3 or 5 tiles:
// 1 channel at K = 16, 2 at 8, 4 at 12, 8 at 10), so both taps of an output meet inside it - and a run of whole columns (grid.y). Its weight slab
// [IC][16 NTG] is fetched once into LDS (n past OC K zero-filled) and reused for every position it walks. The run is walked in rounds of 64 positions
// in increasing p; in a round wave v owns the 16 positions of tile v against all NTG n tiles over all of IC: no cross-wave reduction, one order of
// sums. One MFMA step: lane (r = lane & 15, g = lane >> 4) feeds x of position r at ic kb + g on the A side and w[kb + g][16 nt + r] on the B side,
// and holds Z[position g + 4 q][n r], q = 0..3 (the f64 lane map at the top of hip_mm_tile.h). The activations are read as they are, eight steps ahead.
//
// The rounded taps of a round meet in LDS (zb, row 0 = the last position of the round before: the tap carry - a run starts at a column's l = 0, so a
// round never needs a position its workgroup did not compute, and no halo is recomputed). After a barrier the 256 threads walk (channel, position, j)
// with t = l s0 + j fastest, which is contiguous in out and prev. A column's old tail is read into LDS (tb) BEFORE that barrier, in the round that
// holds its l = 0; the new tail is stored behind the barrier of the round that holds its l = L - 1, which is the same round or a later one.
//
// A column's bits depend on the layer and its own values only: every Z element is one wave's own sum in an order fixed by IC, and nothing else is
// shared between positions. Rows past the run's end are clamped on load and channels past OC read zero weights; neither is stored. No workgroup
// waits for another.
#pragma once

typedef double ctm_f64x4 __attribute__((ext_vector_type(4)));
typedef float ctm_f32x4 __attribute__((ext_vector_type(4)));
#define CTM_ROWS 64        // positions of a round: one 16-row tile per wave
#define CTM_TARGET_WGS 512 // the column split stops once the grid holds this many workgroups

// floats of LDS: the slab, the rounded taps of a round + the carry row, the old tails of a round
static size_t ctm_lds_floats(int NW, int IC) { return (size_t) NW * IC + (size_t) (CTM_ROWS + 1) * NW + (size_t) CTM_ROWS * NW / 2; }

template <int NTG>
__global__ void __launch_bounds__(256) convtr_cols_mfma_kernel(const float * __restrict__ w, const float * __restrict__ x, float * prev, const float * __restrict__ bias,
                                                               float * __restrict__ out, int K, int s0, int IC, int OC, int L, int B, int cols_per_wg, int pre_elu) {
    extern __shared__ float ctm_lds[];
    constexpr int NW = NTG * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int N = OC * K, CG = NW / K, n0 = blockIdx.x * NW, oc0 = blockIdx.x * CG;
    const int RJ = CTM_ROWS * s0;                       // (position, j) pairs of a full round
    const int64_t OLf = (int64_t) (L + 1) * s0, OL = (int64_t) L * s0;
    float * wl = ctm_lds;                               // [IC][NW]
    float * zb = wl + (size_t) IC * NW;                 // [1 + CTM_ROWS][NW]
    float * tb = zb + (CTM_ROWS + 1) * NW;              // [CG][RJ]

    for (int i = tid; i < IC * (NW / 4); i += 256) {
        const int ic = i / (NW / 4), n = n0 + (i % (NW / 4)) * 4;   // (N % 4 == 0: a quad is inside the weight row or past it)
        ctm_f32x4 v = { 0.f, 0.f, 0.f, 0.f };
        if (n < N) v = __builtin_nontemporal_load((const ctm_f32x4 *) (w + (int64_t) ic * N + n));
        *(ctm_f32x4 *) (wl + ic * NW + (n - n0)) = v;
    }
    __syncthreads();

    const int b_first = blockIdx.y * cols_per_wg, b_end = min(B, b_first + cols_per_wg);
    const int p_end = b_end * L;
    for (int P0 = b_first * L; P0 < p_end; P0 += CTM_ROWS) {
        const int nrows = min(CTM_ROWS, p_end - P0);
        // the old tails of the columns that begin in this round
        for (int rj = tid; rj < nrows * s0; rj += 256) {
            const int row = rj / s0, j = rj - row * s0, p = P0 + row, b = p / L;
            if (p - b * L != 0) continue;
            for (int c = 0; c < CG && oc0 + c < OC; c++) tb[c * RJ + rj] = prev[((int64_t) b * OC + oc0 + c) * OLf + OL + j];
        }
        // wave's tile: 16 positions x NW taps over all of IC
        if (wave * 16 < nrows) {
            const int p = min(P0 + wave * 16 + r, p_end - 1), b = p / L;
            const float * xp = x + (int64_t) b * IC * L + (p - b * L) + (int64_t) g * L;   // + ic L: lane's ic = kb + 4 j + g
            ctm_f64x4 acc[NTG];
#pragma unroll
            for (int nt = 0; nt < NTG; nt++) acc[nt] = ctm_f64x4{ 0, 0, 0, 0 };
            float xn[8];
#pragma unroll
            for (int j = 0; j < 8; j++) xn[j] = xp[(int64_t) (4 * j) * L];
            for (int kb = 0; kb < IC; kb += 32) {
                float xc[8];
#pragma unroll
                for (int j = 0; j < 8; j++) xc[j] = xn[j];
                if (kb + 32 < IC) {
#pragma unroll
                    for (int j = 0; j < 8; j++) xn[j] = xp[(int64_t) (kb + 32 + 4 * j) * L];
                }
                if (pre_elu) {
#pragma unroll
                    for (int j = 0; j < 8; j++) xc[j] = xc[j] > 0.f ? xc[j] : expm1f(xc[j]);
                }
                const float * wr = wl + (kb + g) * NW + r;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const double a = (double) xc[j];
#pragma unroll
                    for (int nt = 0; nt < NTG; nt++) acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double) wr[4 * j * NW + nt * 16], acc[nt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int nt = 0; nt < NTG; nt++)
#pragma unroll
                for (int q = 0; q < 4; q++) zb[(1 + wave * 16 + g + 4 * q) * NW + nt * 16 + r] = (float) acc[nt][q];
        }
        __syncthreads();
        // overlap add, tail, bias: t = l s0 + j runs along the threads
        for (int rj = tid; rj < nrows * s0; rj += 256) {
            const int row = rj / s0, j = rj - row * s0, p = P0 + row, b = p / L, l = p - b * L;
            const float * zc = zb + (row + 1) * NW, * zp = zb + row * NW;
            for (int c = 0; c < CG && oc0 + c < OC; c++) {
                const int oc = oc0 + c;
                const float lo = zc[c * K + j], hi = zc[c * K + s0 + j];
                const float y = l > 0 ? zp[c * K + s0 + j] + lo : lo + tb[c * RJ + rj];
                float * pv = prev + ((int64_t) b * OC + oc) * OLf + (int64_t) l * s0 + j;
                pv[0] = y;
                if (l == L - 1) pv[s0] = hi;
                out[((int64_t) b * OC + oc) * OL + (int64_t) l * s0 + j] = bias ? y + bias[oc] : y;
            }
        }
        const float carry = tid < NW ? zb[CTM_ROWS * NW + tid] : 0.f;   // (read by the next round only behind a full one)
        __syncthreads();
        if (tid < NW) zb[tid] = carry;
    }
}
