// valu_issue.hip -- for how many cycles does a wave64 integer VALU instruction hold its SIMD on gfx950?
// (the sweep's VALU floor and tools/sq_summary.py's valu_busy both assume a figure.)
//
// One workgroup -- one CU's worth of waves -- of 4 x W waves, W = 1, 2, 4 waves per SIMD.  Every wave
// runs eight independent chains of one instruction (v_xor_b32, v_ffbl_b32, v_min3_u32, v_and_or_b32:
// the sweep's step), 64 instructions per loop round, between two reads of s_memtime.  With the SIMD
// held H cycles per instruction, a wave's instruction takes max(H, its own issue interval) cycles at
// W = 1 and W x H once the SIMD is the limit: H is the slope over W.
//   hipcc -O3 --offload-arch=gfx950 tools/valu_issue.hip -o tools/valu_issue && tools/valu_issue
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

#define ROUNDS 8  // rounds of the eight chains per loop iteration

template <int OP>
__global__ void valu_issue(unsigned long long* out, int iters) {
  uint32_t a[8];
  const uint32_t s = threadIdx.x | 1u, c = threadIdx.x * 2654435761u;
  for (int j = 0; j < 8; j++) a[j] = c + 0x9e3779b9u * (j + 1);
  __syncthreads();
  unsigned long long t0, t1;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0));
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int r = 0; r < ROUNDS; r++)
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (OP == 0) asm volatile("v_xor_b32_e32 %0, %0, %1" : "+v"(a[j]) : "v"(s));
        if (OP == 1) asm volatile("v_ffbl_b32_e32 %0, %0" : "+v"(a[j]));
        if (OP == 2) asm volatile("v_min3_u32 %0, %0, %1, %2" : "+v"(a[j]) : "v"(s), "v"(c));
        if (OP == 3) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(a[j]) : "v"(c), "v"(s));
      }
  }
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1));
  uint32_t x = 0;
  for (int j = 0; j < 8; j++) x ^= a[j];
  if ((threadIdx.x & 63u) == 0) out[threadIdx.x >> 6] = t1 - t0;
  if (x == 0x12345u && iters < 0) out[0] = x;  // (keeps the chains)
}

int main() {
  const int iters = 4096;
  const char* names[4] = {"v_xor_b32", "v_ffbl_b32", "v_min3_u32", "v_and_or_b32"};
  void (*kern[4])(unsigned long long*, int) = {valu_issue<0>, valu_issue<1>, valu_issue<2>, valu_issue<3>};
  unsigned long long *d, h[16];
  if (hipMalloc(&d, sizeof h) != hipSuccess) return 1;
  printf("%-14s %s\n", "instruction", "waves/SIMD  s_memtime ticks per wave (min - max)  per wave instruction  per instruction of the SIMD");
  for (int op = 0; op < 4; op++)
    for (int w = 1; w <= 4; w *= 2) {
      unsigned long long lo = ~0ull, hi = 0;
      for (int rep = 0; rep < 3; rep++) {  // the last repeat counts (the first warms the instruction cache)
        hipLaunchKernelGGL(kern[op], dim3(1), dim3(256 * w), 0, 0, d, iters);
        if (hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return 1;
      }
      for (int i = 0; i < 4 * w; i++) { lo = h[i] < lo ? h[i] : lo; hi = h[i] > hi ? h[i] : hi; }
      const double n = (double)iters * ROUNDS * 8;
      printf("%-14s %d           %llu - %llu   %.3f   %.3f\n", names[op], w, lo, hi, hi / n, hi / n / w);
    }
  (void)hipFree(d);
  return 0;
}
