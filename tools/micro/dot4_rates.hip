// Dev tool (GPU): issue rate of the signed 4 x 8-bit dot product against the integer instructions the ball query's node
// test could be made of instead (inline assembly, so nothing is folded).  Every wave runs a dependent chain; with eight
// waves per SIMD the figure is the issue rate, not the latency.
// hipcc --offload-arch=gfx950 -O3 -o dot4_rates tools/micro/dot4_rates.hip && ./dot4_rates
#include <hip/hip_runtime.h>
#include <cstdio>
#define N_IT 4096
template <int OP>
__global__ void k(int *out, int a) {
  int x = a + threadIdx.x;
  int acc = threadIdx.x;
  for (int it = 0; it < N_IT; it++) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      if (OP == 0) asm volatile("v_sub_u32 %0, %0, %1" : "+v"(acc) : "v"(x));
      if (OP == 1) asm volatile("v_dot4c_i32_i8 %0, %1, %1" : "+v"(acc) : "v"(x));
      if (OP == 2) asm volatile("v_dot4_i32_i8 %0, %1, %1, %0" : "+v"(acc) : "v"(x));
      if (OP == 3) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(acc) : "v"(x));
      if (OP == 4) asm volatile("v_mad_u32_u24 %0, %1, %1, %0" : "+v"(acc) : "v"(x));
      if (OP == 5) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(acc) : "v"(x));
      if (OP == 6) asm volatile("v_bfe_i32 %0, %0, 8, 8" : "+v"(acc));
      if (OP == 7) asm volatile("v_min3_u32 %0, %0, %1, %1" : "+v"(acc) : "v"(x));
    }
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}
template <int OP>
void run(const char *name, int *d) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const int blocks = 256 * 4 * 2, threads = 256;
  hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(threads), 0, 0, d, 3);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0);
  hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(threads), 0, 0, d, 3);
  (void)hipEventRecord(e1);
  (void)hipEventSynchronize(e1);
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double groups = (double)blocks * threads / 64 * N_IT * 8;
  printf("%-28s %7.3f ms  %5.2f clk per instruction and SIMD at 2.4 GHz\n", name, ms, ms * 1e-3 * 2.4e9 / (groups / 1024));
}
int main() {
  int *d;
  if (hipMalloc(&d, sizeof(int) * 256 * 4 * 2 * 256) != hipSuccess) return 1;
  run<0>("v_sub_u32", d);
  run<1>("v_dot4c_i32_i8", d);
  run<2>("v_dot4_i32_i8", d);
  run<3>("v_mul_u32_u24", d);
  run<4>("v_mad_u32_u24", d);
  run<5>("v_mul_lo_u32", d);
  run<6>("v_bfe_i32", d);
  run<7>("v_min3_u32", d);
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
