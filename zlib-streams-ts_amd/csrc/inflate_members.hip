// inflate_members.hip -- a gzip file's members found from its bytes and decoded together (DESIGN 4.14;
// zlib's gz_look, gzread.c: behind a member's trailer the next member starts where 1f 8b follows).
//   zs_k_members_scan    the candidates: every offset q >= 1 whose four bytes are 1f 8b 08 and a flag byte
//                        without a reserved bit.  Two passes over the bytes, <false> counts per tile and
//                        <true> emits, with the tiles' prefix sums (zs_k_flush_tiles) between them: every
//                        tile owns its part of the list, so the list is in increasing order and the same
//                        on every run.
//   zs_k_members_size    one lane per start (a stream's offset 0 or a candidate): the member sized by
//                        zs_members.h, stopped at candidate j + sync_pass + 1 of its stream at the latest
//   zs_k_members_tail    the starts a bound stopped (true members that hold more than sync_pass false
//                        candidates): one lane each, unbounded to the stream's end.  The host then plans
//                        again from the records it has; every round settles at least one member of each
//                        listed stream and costs one synchronisation of the stream.
//   (the members decode as the members of one gzip batch on the caller's input, by the decoders as they
//   are; zs_k_restart_place moves them on the staging route)
//   zs_k_members_stitch  per stream: the first member that did not end cleanly; the stream's status,
//                        lengths and the length its check value is taken over
// No atomics, no waits between workgroups.  The members are planned on the host (zs_plan_members).
#include "zs_kernels.h"
#include "zs_inflate.h"
#include "zs_members.h"

// the stream that holds tile t: the last s with tile[s] <= t (tile: n + 1 prefix sums, tile[n] > t)
static __device__ __forceinline__ uint32_t zs_members_find(const uint32_t* __restrict__ tile, uint32_t n, uint32_t t) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tile[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One workgroup step scans ZS_SYNC_TILE bytes of one stream, an aligned 16-byte unit per lane; the grid
// strides over the call's tiles (stile: prefix sums of the streams' tiles).  tcount: T + 1 values -- the
// count pass writes every tile's count and 0 behind them, zs_k_flush_tiles turns them into the tiles'
// first indices and the total, the emit pass reads those.  cand: the list, `cap` entries (an index past
// it is not written: the host reads the total, grows the list and runs the pass again).
template <bool EMIT>
__global__ __launch_bounds__(256) void zs_k_members_scan(const uint8_t* __restrict__ in,
                                                         const uint64_t* __restrict__ in_off,
                                                         const uint32_t* __restrict__ in_len,
                                                         const uint32_t* __restrict__ stile, uint32_t n,
                                                         uint64_t* __restrict__ tcount, uint32_t* __restrict__ cand,
                                                         uint64_t cap) {
  __shared__ uint32_t wsum[4];
  const uint32_t T = stile[n];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (!EMIT && blockIdx.x == 0 && threadIdx.x == 0) tcount[T] = 0;
  for (uint32_t t = blockIdx.x; t < T; t += gridDim.x) {
    const uint32_t s = zs_members_find(stile, n, t);
    const uint64_t u = (uint64_t)(t - stile[s]) * (ZS_SYNC_TILE / 16u) + threadIdx.x;
    int64_t q0;
    uint32_t mask = zs_members_unit(in + in_off[s], in_len[s], u, q0);
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
template __global__ void zs_k_members_scan<false>(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                                                  uint32_t, uint64_t*, uint32_t*, uint64_t);
template __global__ void zs_k_members_scan<true>(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                                                 uint32_t, uint64_t*, uint32_t*, uint64_t);

// Lane x of the launch: x < n is stream x's offset 0, x = n + k candidate k of the list.  tpre: the
// tiles' first indices and, behind them, the candidates' count C (more than `cap`: the list is not
// complete and nothing runs).  Candidate k belongs to the stream s with tpre[stile[s]] <= k <
// tpre[stile[s + 1]].  A lane started at candidate j of its stream (offset 0: j = -1) is bounded by
// candidate j + pass + 1, or by the stream's end: every input byte is decoded by at most pass + 1 bounded
// lanes and the kernel's work is linear in the call's bytes, whatever the bytes are.  ZS_SYNC_LANES
// lanes to a workgroup, their tables in LDS, as zs_k_sync_size.
__global__ __launch_bounds__(ZS_SYNC_LANES) void zs_k_members_size(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len,
    const uint32_t* __restrict__ stile, uint32_t n, const uint64_t* __restrict__ tpre,
    const uint32_t* __restrict__ cand, uint64_t cap, uint32_t pass, zs_sync_rec* __restrict__ rec) {
  __shared__ zs_sync_tabs tabs[ZS_SYNC_LANES];
  const uint64_t x = (uint64_t)blockIdx.x * ZS_SYNC_LANES + threadIdx.x;
  const uint64_t C = tpre[stile[n]];
  if (C > cap || x >= n + C) return;
  uint32_t s, start;
  uint64_t bi;  // the bounding candidate's index among the stream's
  if (x < n) {
    s = (uint32_t)x;
    start = 0;
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
  rec[x] = zs_members_size(in + in_off[s], in_len[s], start, bound, tabs[threadIdx.x]);
}

// One lane per listed start (tstream, tstart: m of them), unbounded: the member sized to the stream's end.
__global__ __launch_bounds__(ZS_SYNC_LANES) void zs_k_members_tail(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len,
    const uint32_t* __restrict__ tstream, const uint32_t* __restrict__ tstart, uint32_t m,
    zs_sync_rec* __restrict__ rec) {
  __shared__ zs_sync_tabs tabs[ZS_SYNC_LANES];
  const uint32_t x = blockIdx.x * ZS_SYNC_LANES + threadIdx.x;
  if (x >= m) return;
  const uint32_t s = tstream[x];
  rec[x] = zs_members_size(in + in_off[s], in_len[s], tstart[x], in_len[s], tabs[threadIdx.x]);
}

// One wave per stream.  A lane per member finds the first member that did not end with Z_STREAM_END, a
// round of 64 at a time with the first failure carried across rounds.  Lane 0 then writes the stream's
// fields.  All members ended: Z_STREAM_END, the last member's phase and message, out_len = the total,
// consumed = the offset behind the last trailer.  Else the failing member's status, phase and message
// (the decoder's own, for the bytes from its start on), out_len = its out_pos (the members before it
// are complete), consumed = its start.  cklen[s]: the bytes the stream's check value is taken over --
// the total, or 0 for a stream that failed (the crc32 of no bytes is 0).
// trusted (null in the _members calls; the _bgzf calls'): one byte per member, set where the
// member's room was its header's ISIZE.  Such a member that ends with the capacity outcome (Z_BUF_ERROR,
// "output capacity exceeded") produced more than its ISIZE says: it is reported as Z_DATA_ERROR, "incorrect
// length check" -- zlib's words for an ISIZE that does not match -- so that the caller can tell it from a
// capacity of their own that is too small.  (Z_BUF_ERROR with no message is input that ended early, a BSIZE
// that is too small: it stays as the decoder reports it.)
__global__ __launch_bounds__(64) void zs_k_members_stitch(
    const uint32_t* __restrict__ rfirst, const uint32_t* __restrict__ soff, const uint32_t* __restrict__ opos,
    const int32_t* __restrict__ seg_status, const int32_t* __restrict__ seg_phase, const int32_t* __restrict__ seg_msg,
    const uint32_t* __restrict__ seg_len, const uint32_t* __restrict__ seg_used, uint32_t n,
    int32_t* __restrict__ status, int32_t* __restrict__ phase, int32_t* __restrict__ msg, uint32_t* __restrict__ out_len,
    uint32_t* __restrict__ consumed, uint32_t* __restrict__ cklen, const uint8_t* __restrict__ trusted) {
  const uint32_t s = blockIdx.x;
  if (s >= n) return;
  const uint32_t g0 = rfirst[s], g1 = rfirst[s + 1];
  uint32_t bad = 0xffffffffu;
  for (uint32_t base = g0; base < g1 && bad == 0xffffffffu; base += 64u) {
    const uint32_t g = base + threadIdx.x;
    const bool fails = g < g1 && seg_status[g] != ZS_Z_STREAM_END;
    const unsigned long long m = __ballot(fails);
    if (m) bad = base + (uint32_t)__ffsll(m) - 1u;
  }
  if (threadIdx.x != 0) return;
  const bool ok = bad == 0xffffffffu;
  const uint32_t g = ok ? g1 - 1u : bad;
  const bool lied = trusted && trusted[g] && seg_status[g] == ZS_Z_BUF_ERROR && seg_msg[g] == ZS_MSG_CAPACITY;
  status[s] = lied ? ZS_Z_DATA_ERROR : seg_status[g];
  phase[s] = lied ? ZS_PHASE_PROCESS_ : seg_phase[g];
  msg[s] = lied ? ZS_MSG_LENGTH_CHECK : seg_msg[g];
  out_len[s] = ok ? opos[g] + seg_len[g] : opos[g];
  consumed[s] = ok ? soff[g] + seg_used[g] : soff[g];
  cklen[s] = ok ? opos[g] + seg_len[g] : 0u;
}
