// Row converters of the BF16 / F16 batched mat-muls (hip_mm_tile.h), included from hip_kernels_fused.hip: the T activation rows, F32, rounded to the
// weight's type - what ggml's generic BF16 / F16 product multiplies - dense [T][K] in the workspace (K % 8 == 0). Both forms read the same workspace.
#pragma once

template <int WT> __device__ __forceinline__ uint16_t mmf_round(float v) { return WT == GGML_TYPE_F16 ? f2h(v) : f2bf(v); }
template <int WT> __device__ __forceinline__ u32x4 mmf_pack8(const float v[8]) {
    u32x4 o;
    o.x = (uint32_t) mmf_round<WT>(v[0]) | ((uint32_t) mmf_round<WT>(v[1]) << 16); o.y = (uint32_t) mmf_round<WT>(v[2]) | ((uint32_t) mmf_round<WT>(v[3]) << 16);
    o.z = (uint32_t) mmf_round<WT>(v[4]) | ((uint32_t) mmf_round<WT>(v[5]) << 16); o.w = (uint32_t) mmf_round<WT>(v[6]) | ((uint32_t) mmf_round<WT>(v[7]) << 16);
    return o;
}

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
