// zs_flush_scan.h -- the workgroup scan of the per-segment layouts (deflate_flush.hip, deflate_bgzf.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// exclusive scan of v over the 256-thread workgroup; total: the workgroup's sum
static __device__ __forceinline__ uint64_t zs_flush_scan256(uint64_t v, uint64_t* tmp, uint64_t& total) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint64_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(x, d, 64);
    if (lane >= (uint32_t)d) x += y;
  }
  if (lane == 63) tmp[wv] = x;
  __syncthreads();
  uint64_t pre = 0;
  for (uint32_t i = 0; i < wv; i++) pre += tmp[i];
  total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
  return pre + x - v;
}
