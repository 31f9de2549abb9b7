// inflate_sync.hip -- a stream's restart points found from its bytes (inflateSync /
// syncsearch, inflate.ts:1267-1337: the reference looks for 00 00 FF FF and resets the stream behind it).
//   zs_k_sync_first   device entry only: every stream's first point, the wrapper's header length
//                     (zs_wrapper_header_len_of, the parse the host entries run on their own bytes)
//   zs_k_sync_scan    the candidates: every offset q with in[q-4..q) == 00 00 FF FF behind the first
//                     point.  Two passes over the bytes, <false> counts per tile and <true> emits, with
//                     the tiles' prefix sums (zs_k_flush_tiles) between them (zs_cand.h)
//   zs_k_sync_size    one lane per start (a first point or a candidate): the count-only decode of
//                     zs_sync.h, stopped at candidate j + sync_pass + 1 of its stream at the latest
//   zs_k_sync_tail    the few chains that end at a lane the bound stopped: that lane's start once more, to
//                     the stream's end, for the reach of the whole tail
// No atomics, no waits between workgroups.  The points are planned on the host (zs_plan_sync) and the
// restart path (inflate_restart.hip) decodes from them.
#include "zs_kernels.h"
#include "zs_inflate.h"
#include "zs_sync.h"
#include "zs_cand.h"

__global__ void zs_k_sync_first(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                const uint32_t* __restrict__ in_len, int wbits, uint32_t n,
                                uint32_t* __restrict__ first) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  // (a gzip header that is malformed or does not fit gives 0, a zlib stream shorter than its header
  // its length: both fail the header check of zs_k_restart_stitch)
  first[s] = min(zs_wrapper_header_len_of(wbits, in + in_off[s], in_len[s]), in_len[s]);
}

// The candidates' two passes (zs_cand_scan), over zs_sync_unit behind each stream's first point.
template <bool EMIT>
__global__ __launch_bounds__(256) void zs_k_sync_scan(const uint8_t* __restrict__ in,
                                                      const uint64_t* __restrict__ in_off,
                                                      const uint32_t* __restrict__ in_len,
                                                      const uint32_t* __restrict__ first,
                                                      const uint32_t* __restrict__ stile, uint32_t n,
                                                      uint64_t* __restrict__ tcount, uint32_t* __restrict__ cand,
                                                      uint64_t cap) {
  zs_cand_scan<EMIT>(stile, n, tcount, cand, cap, [&](uint32_t s, uint64_t u, int64_t& q0) {
    return zs_sync_unit(in + in_off[s], in_len[s], first[s], u, q0);
  });
}
template __global__ void zs_k_sync_scan<false>(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                                               const uint32_t*, uint32_t, uint64_t*, uint32_t*, uint64_t);
template __global__ void zs_k_sync_scan<true>(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                                              const uint32_t*, uint32_t, uint64_t*, uint32_t*, uint64_t);

// Lane x of the launch (zs_cand_lookup): stream x's first point or candidate x - n, bounded by zs_cand_bound.
// tpre's last value is the candidates' count C (more than `cap`: the list is not complete and nothing runs).
// ZS_SYNC_LANES lanes to a workgroup: their tables are 34 KB of LDS, and a lane's own time is the kernel's
// (DESIGN 5).
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
  const zs_cand_lane l = zs_cand_lookup(x, n, stile, tpre);
  const uint32_t s = l.s, start = l.k == ZS_CAND_FIRST ? min(first[s], in_len[s]) : cand[l.k];
  const uint32_t bound = zs_cand_bound(l, stile, tpre, cand, pass, in_len[s]);
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
