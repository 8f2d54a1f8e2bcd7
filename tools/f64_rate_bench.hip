// f64_rate_bench.hip — issue rates of v_fma_f32, v_fma_f64 and v_cvt_f64_f32 on every SIMD (8 independent chains per wave), and of
// the two per-coefficient mixes of lr_project_kernel (csrc/rpgp_lowrank.hip): float32 recurrence + widening + float64 accumulate
// against two float64 FMAs (profiles/lowrank_mvm_roundtrip_f64_rates.txt).
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/f64_rate_bench.hip -o tools/f64_rate_bench
#include <hip/hip_runtime.h>
#include <stdio.h>
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
template <int MODE>
__global__ __launch_bounds__(256) void rate_kernel(float *out, float seed, int iters) {
  float f[8]; double d[8];
  const double x = seed, y = seed * 0.5;
  const float xf = seed, yf = seed * 0.5f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { f[i] = seed + i + threadIdx.x; d[i] = f[i]; }
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (MODE == 0) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(f[i]) : "v"(xf), "v"(yf));
        if (MODE == 1) asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(d[i]) : "v"(x), "v"(y));
        if (MODE == 2) asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[i]) : "v"(f[i]));
        if (MODE == 3) { asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(f[i]) : "v"(xf), "v"(yf));
                         asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[i]) : "v"(f[i]));
                         asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(d[(i + 4) & 7]) : "v"(x), "v"(y)); }
        if (MODE == 4) { asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(d[i]) : "v"(x), "v"(y));
                         asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(d[(i + 4) & 7]) : "v"(x), "v"(y)); }
      }
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += f[i] + (float)d[i];
  if (s == 12345.678f) out[threadIdx.x] = s;
}
template <int MODE> int run(const char *name, int per, int blocks, float *out) {
  const int iters = 2000;
  hipEvent_t e0, e1;
  CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
  hipLaunchKernelGGL(rate_kernel<MODE>, dim3(blocks), dim3(256), 0, 0, out, 1.0f, 10);
  CHK(hipDeviceSynchronize());
  CHK(hipEventRecord(e0));
  hipLaunchKernelGGL(rate_kernel<MODE>, dim3(blocks), dim3(256), 0, 0, out, 1.0f, iters);
  CHK(hipEventRecord(e1));
  CHK(hipEventSynchronize(e1));
  float ms = 0.f;
  CHK(hipEventElapsedTime(&ms, e0, e1));
  const double winstr = (double)blocks * 4 * iters * 16 * 8 * per;       // wave-instructions
  printf("%-44s blocks=%5d  time=%8.3f ms  ns per wave-instr per SIMD=%7.3f  (cycles at 2.4 GHz: %5.2f)\n", name, blocks, ms,
         ms * 1e6 / (winstr / 1024.0), ms * 1e6 / (winstr / 1024.0) * 2.4);
  return 0;
}
int main() {
  float *out;
  CHK(hipMalloc(&out, 4096));
  for (int blocks : {256, 1024, 2048}) {
    if (run<0>("v_fma_f32", 1, blocks, out)) return 1;
    if (run<1>("v_fma_f64", 1, blocks, out)) return 1;
    if (run<2>("v_cvt_f64_f32", 1, blocks, out)) return 1;
    if (run<3>("v_fma_f32 + v_cvt_f64_f32 + v_fma_f64 (parent)", 3, blocks, out)) return 1;
    if (run<4>("2 v_fma_f64 (this change)", 2, blocks, out)) return 1;
  }
  CHK(hipFree(out));
  return 0;
}
