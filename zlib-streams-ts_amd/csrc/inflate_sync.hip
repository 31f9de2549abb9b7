// inflate_sync.hip -- a stream's restart points found from its bytes (inflateSync /
// syncsearch, inflate.ts:1267-1337: the reference looks for 00 00 FF FF and resets the stream behind it).
//   zs_k_sync_first   device entry only: every stream's first point, the wrapper's header length
//                     (zs_wrapper_header_len_of, the parse the host entries run on their own bytes)
//   zs_k_sync_scan    the candidates: every offset q with in[q-4..q) == 00 00 FF FF behind the first
//                     point.  Two passes over the bytes, <false> counts per tile and <true> emits, with
//                     the tiles' prefix sums (zs_k_flush_tiles) between them: every tile owns its part
//                     of the list, so the list is in increasing order and the same on every run.
//   zs_k_sync_size    one lane per start (a first point or a candidate): the count-only decode of
//                     zs_sync.h, stopped at candidate j + sync_pass + 1 of its stream at the latest
//   zs_k_sync_tail    the few chains that end at a lane the bound stopped: that lane's start once more, to
//                     the stream's end, for the reach of the whole tail
// No atomics, no waits between workgroups.  The points are planned on the host (zs_plan_sync) and the
// restart path (inflate_restart.hip) decodes from them.
#include "zs_kernels.h"
#include "zs_inflate.h"
#include "zs_sync.h"

// the stream that holds tile t: the last s with tile[s] <= t (tile: n + 1 prefix sums, tile[n] > t)
static __device__ __forceinline__ uint32_t zs_sync_find(const uint32_t* __restrict__ tile, uint32_t n, uint32_t t) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tile[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void zs_k_sync_first(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                const uint32_t* __restrict__ in_len, int wbits, uint32_t n,
                                uint32_t* __restrict__ first) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  // (a gzip header that is malformed or does not fit gives 0, a zlib stream shorter than its header
  // its length: both fail the header check of zs_k_restart_stitch)
  first[s] = min(zs_wrapper_header_len_of(wbits, in + in_off[s], in_len[s]), in_len[s]);
}

// One workgroup step scans ZS_SYNC_TILE bytes of one stream, an aligned 16-byte unit per lane; the grid
// strides over the call's tiles (stile: prefix sums of the streams' tiles), so a 20-byte stream takes
// one step and a 64 MiB stream 16,384 of them.  tcount: T + 1 values -- the count pass writes every
// tile's count and 0 behind them, zs_k_flush_tiles turns them into the tiles' first indices and the
// total, the emit pass reads those.  cand: the list, `cap` entries (an index past it is not written:
// the host reads the total, grows the list and runs the pass again).
template <bool EMIT>
__global__ __launch_bounds__(256) void zs_k_sync_scan(const uint8_t* __restrict__ in,
                                                      const uint64_t* __restrict__ in_off,
                                                      const uint32_t* __restrict__ in_len,
                                                      const uint32_t* __restrict__ first,
                                                      const uint32_t* __restrict__ stile, uint32_t n,
                                                      uint64_t* __restrict__ tcount, uint32_t* __restrict__ cand,
                                                      uint64_t cap) {
  __shared__ uint32_t wsum[4];
  const uint32_t T = stile[n];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (!EMIT && blockIdx.x == 0 && threadIdx.x == 0) tcount[T] = 0;
  for (uint32_t t = blockIdx.x; t < T; t += gridDim.x) {
    const uint32_t s = zs_sync_find(stile, n, t);
    const uint64_t u = (uint64_t)(t - stile[s]) * (ZS_SYNC_TILE / 16u) + threadIdx.x;
    int64_t q0;
    uint32_t mask = zs_sync_unit(in + in_off[s], in_len[s], first[s], u, q0);
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
template __global__ void zs_k_sync_scan<false>(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                                               const uint32_t*, uint32_t, uint64_t*, uint32_t*, uint64_t);
template __global__ void zs_k_sync_scan<true>(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                                              const uint32_t*, uint32_t, uint64_t*, uint32_t*, uint64_t);

// Lane x of the launch: x < n is stream x's first point, x = n + k candidate k of the list.  tpre: the
// tiles' first indices and, behind them, the candidates' count C (more than `cap`: the list is not
// complete and nothing runs).  Candidate k belongs to the stream s with tpre[stile[s]] <= k <
// tpre[stile[s + 1]].  A lane started at candidate j of its stream (the first point: j = -1) is bounded
// by candidate j + pass + 1, or by the stream's end: every input byte is decoded by at most pass + 1
// lanes and the kernel's work is linear in the call's bytes, whatever the bytes are.  ZS_SYNC_LANES lanes
// to a workgroup: their tables are 34 KB of LDS, and a lane's own time is the kernel's.
__global__ __launch_bounds__(ZS_SYNC_LANES) void zs_k_sync_size(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                     const uint32_t* __restrict__ in_len,
                                                     const uint32_t* __restrict__ first,
                                                     const uint32_t* __restrict__ stile, uint32_t n,
                                                     const uint64_t* __restrict__ tpre, const uint32_t* __restrict__ cand,
                                                     uint64_t cap, uint32_t pass, zs_sync_rec* __restrict__ rec) {
  __shared__ zs_sync_tabs tabs[ZS_SYNC_LANES];
  const uint64_t x = (uint64_t)blockIdx.x * ZS_SYNC_LANES + threadIdx.x;
  const uint64_t C = tpre[stile[n]];
  if (C > cap || x >= n + C) return;
  uint32_t s, start;
  uint64_t bi;  // the bounding candidate's index among the stream's
  if (x < n) {
    s = (uint32_t)x;
    start = min(first[s], in_len[s]);
    bi = pass;
  } else {
    const uint64_t k = x - n;
    uint32_t lo = 0, hi = n;  // tpre[stile[lo]] <= k < tpre[stile[hi]]
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (tpre[stile[mid]] <= k) lo = mid;
      else hi = mid;
    }
    s = lo;
    start = cand[k];
    bi = k - tpre[stile[s]] + pass + 1u;
  }
  const uint64_t c0 = tpre[stile[s]], c1 = tpre[stile[s + 1]];
  const uint32_t bound = bi < c1 - c0 ? cand[c0 + bi] : in_len[s];
  rec[x] = zs_sync_size(in + in_off[s], in_len[s], start, bound, tabs[threadIdx.x]);
}

// A chain that ends at a PASSED lane makes that lane's start the last point, and the record holds the
// reach only up to where the bound stopped it.  One lane per such tail (tstream, tstart: m of them)
// decodes it once more to the stream's end without stopping where it lands; the host takes the reach.
// At most one tail per stream, each read once: linear in the call's bytes as the bounded lanes are.
__global__ __launch_bounds__(ZS_SYNC_LANES) void zs_k_sync_tail(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                     const uint32_t* __restrict__ in_len,
                                                     const uint32_t* __restrict__ tstream,
                                                     const uint32_t* __restrict__ tstart, uint32_t m,
                                                     zs_sync_rec* __restrict__ rec) {
  __shared__ zs_sync_tabs tabs[ZS_SYNC_LANES];
  const uint32_t x = blockIdx.x * ZS_SYNC_LANES + threadIdx.x;
  if (x >= m) return;
  const uint32_t s = tstream[x];
  rec[x] = zs_sync_size(in + in_off[s], in_len[s], tstart[x], in_len[s], tabs[threadIdx.x], true);
}
