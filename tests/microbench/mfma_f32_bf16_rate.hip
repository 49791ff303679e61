// Issue rate of v_mfma_f32_16x16x32_bf16 on gfx950: a bare loop of it (four independent accumulator chains per wave, no memory traffic) on every CU.
// Prints TFLOP/s (2 * 16 * 16 * 32 FLOP per instruction) and ns per instruction per SIMD - both measured - and that time in cycles of the device's
// REPORTED maximum clock (hipDeviceProp_t::clockRate; the clock the run sustained is not read, so the cycle figure is an upper bound).
// The companion of mfma_f64_rate.hip for the float-accumulating mat-mul (hip_mm_float_acc.h).
// Build: hipcc --offload-arch=gfx950 -O2 mfma_f32_bf16_rate.hip -o mfma_f32_bf16_rate
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); exit(1); } } while (0)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define CHAINS 4
__global__ void __launch_bounds__(256) k(float * out, int iters, unsigned int a0, unsigned int b0) {
    const u32x4 au = { a0 + threadIdx.x, a0, a0, a0 }, bu = { b0, b0, b0, b0 };   // pairs of small BF16 values
    const bf16x8 a = __builtin_bit_cast(bf16x8, au), b = __builtin_bit_cast(bf16x8, bu);
    f32x4 acc[CHAINS];
    for (int c = 0; c < CHAINS; c++) acc[c] = f32x4{ 0, 0, 0, 0 };
    for (int i = 0; i < iters; i++)
#pragma unroll
        for (int c = 0; c < CHAINS; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[c], 0, 0, 0);
    float s = 0;
    for (int c = 0; c < CHAINS; c++) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    if (s == 12345.678f) out[0] = s;                    // keeps the chains alive; never true
}
int main() {
    hipDeviceProp_t p; CHECK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount, iters = 1 << 14;
    const double ghz = p.clockRate * 1e-6;              // kHz -> GHz
    float * out; CHECK(hipMalloc(&out, 8));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int wps = 1; wps <= 4; wps *= 2) {             // waves per SIMD: workgroups of four waves, wps of them per CU
        const int grid = cus * wps;
        k<<<grid, 256>>>(out, 64, 0x3a003a00u, 0x3b003b00u);   // warm-up
        CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize());
        float best = 1e30f;
        for (int rep = 0; rep < 5; rep++) {
            CHECK(hipEventRecord(e0)); k<<<grid, 256>>>(out, iters, 0x3a003a00u, 0x3b003b00u); CHECK(hipGetLastError()); CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (ms < best) best = ms;
        }
        const double n = (double) grid * 4 * iters * CHAINS, tf = n * 16384 / (best * 1e-3) / 1e12;
        const double per_simd_ns = best * 1e6 / ((double) wps * iters * CHAINS);
        printf("{\"mfma_f32_16x16x32_bf16\": {\"cus\": %d, \"waves_per_simd\": %d, \"ms\": %.3f, \"tflops\": %.2f, \"ns_per_instruction_per_simd\": %.2f, \"reported_max_clock_ghz\": %.2f, \"cycles_at_that_clock\": %.1f}}\n",
               cus, wps, best, tf, per_simd_ns, ghz, per_simd_ns * ghz);
    }
    CHECK(hipFree(out));
    return 0;
}
