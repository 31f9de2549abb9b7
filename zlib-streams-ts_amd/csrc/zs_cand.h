// zs_cand.h -- what the searches that find a stream's pieces from its bytes share on the device (restart
// points, inflate_sync.hip; gzip members, inflate_members.hip; BGZF blocks, inflate_bgzf.hip): the stream of
// a tile, the scan's two passes over a unit rule, and the numbering of the sizing lanes.  The lookups are
// plain C++ (ZS_PLAN_FN), so tools/sync_host, members_host and bgzf_host run the kernels' own.
#ifndef ZS_CAND_H
#define ZS_CAND_H
#include "zs_plan.h"

// the stream that holds tile t: the last s with tile[s] <= t (tile: n + 1 prefix sums, tile[n] > t)
ZS_PLAN_FN uint32_t zs_cand_find(const uint32_t* tile, uint32_t n, uint32_t t) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tile[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Lane x of a sizing launch: x < n starts at stream x's first point, x = n + k at candidate k of the list.
// tpre: the tiles' first indices and, behind them, the candidates' count.  Candidate k belongs to the stream
// s with tpre[stile[s]] <= k < tpre[stile[s + 1]].
#define ZS_CAND_FIRST (~0ull)
struct zs_cand_lane {
  uint32_t s;  // the lane's stream
  uint64_t k;  // its candidate's index in the list, or ZS_CAND_FIRST
  uint64_t j;  // ... and among its stream's, plus one; the first point: 0
};
ZS_PLAN_FN zs_cand_lane zs_cand_lookup(uint64_t x, uint32_t n, const uint32_t* stile, const uint64_t* tpre) {
  if (x < n) return {(uint32_t)x, ZS_CAND_FIRST, 0u};
  const uint64_t k = x - n;
  uint32_t lo = 0, hi = n;  // tpre[stile[lo]] <= k < tpre[stile[hi]]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tpre[stile[mid]] <= k) lo = mid;
    else hi = mid;
  }
  return {lo, k, k - tpre[stile[lo]] + 1u};
}
// ... and its bound: a lane started at candidate j - 1 of its stream (the first point: j = 0) stops at candidate
// j + pass or at the stream's end, so every input byte is decoded by at most pass + 1 bounded lanes and a
// sizing kernel's work is linear in the call's bytes, whatever the bytes are.
ZS_PLAN_FN uint32_t zs_cand_bound(const zs_cand_lane& l, const uint32_t* stile, const uint64_t* tpre, const uint32_t* cand,
                                  uint32_t pass, uint32_t in_len) {
  const uint64_t c0 = tpre[stile[l.s]], c1 = tpre[stile[l.s + 1]];
  const uint64_t bi = l.j + pass;  // the bound's index among the stream's
  return bi < c1 - c0 ? cand[c0 + bi] : in_len;
}

#if defined(__HIPCC__)
// The scan.  One workgroup step covers ZS_SYNC_TILE bytes of one stream, an aligned 16-byte unit per lane; the
// grid strides over the call's tiles (stile: prefix sums of the streams' tiles), so a 20-byte stream takes
// one step and a 64 MiB stream 16,384 of them.  unit(s, u, q0): the mask of stream s's unit u, bit i a
// candidate at q0 + i.  tcount: T + 1 values -- the count pass writes every tile's count and 0 behind them,
// zs_k_flush_tiles turns them into the tiles' first indices and the total, the emit pass reads those: every
// tile owns its part of the list, so the list is in increasing order and the same on every run.  cand: the
// list, `cap` entries (an index past it is not written: the host reads the total, grows the list and runs
// the pass again).  256 threads.
template <bool EMIT, class Unit>
static __device__ __forceinline__ void zs_cand_scan(const uint32_t* __restrict__ stile, uint32_t n,
                                                    uint64_t* __restrict__ tcount, uint32_t* __restrict__ cand,
                                                    uint64_t cap, Unit unit) {
  __shared__ uint32_t wsum[4];
  const uint32_t T = stile[n];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (!EMIT && blockIdx.x == 0 && threadIdx.x == 0) tcount[T] = 0;
  for (uint32_t t = blockIdx.x; t < T; t += gridDim.x) {
    const uint32_t s = zs_cand_find(stile, n, t);
    const uint64_t u = (uint64_t)(t - stile[s]) * (ZS_SYNC_TILE / 16u) + threadIdx.x;
    int64_t q0;
    uint32_t mask = unit(s, u, q0);
    const uint32_t c = (uint32_t)__popc(mask);
    uint32_t x = c;  // the inclusive sum over the wave's lanes up to this one
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63u) wsum[wv] = x;
    __syncthreads();
    if (!EMIT) {
      if (threadIdx.x == 0) tcount[t] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
    } else {
      uint64_t at = tcount[t] + (x - c);
      for (uint32_t k = 0; k < wv; k++) at += wsum[k];
      while (mask) {
        const uint32_t i = (uint32_t)__ffs(mask) - 1u;
        mask &= mask - 1u;
        if (at < cap) cand[at] = (uint32_t)(q0 + (int64_t)i);
        at++;
      }
    }
    __syncthreads();  // wsum is read before the next step rewrites it
  }
}
#endif

#endif
