// inflate_members.hip -- a gzip file's members found from its bytes and decoded together (DESIGN 4.14;
// zlib's gz_look, gzread.c: behind a member's trailer the next member starts where 1f 8b follows).
//   zs_k_members_scan    the candidates: every offset q >= 1 whose four bytes are 1f 8b 08 and a flag byte
//                        without a reserved bit.  Two passes over the bytes, <false> counts per tile and
//                        <true> emits, with the tiles' prefix sums (zs_k_flush_tiles) between them (zs_cand.h)
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
#include "zs_cand.h"

// The candidates' two passes (zs_cand_scan), over zs_members_unit.
template <bool EMIT>
__global__ __launch_bounds__(256) void zs_k_members_scan(const uint8_t* __restrict__ in,
                                                         const uint64_t* __restrict__ in_off,
                                                         const uint32_t* __restrict__ in_len,
                                                         const uint32_t* __restrict__ stile, uint32_t n,
                                                         uint64_t* __restrict__ tcount, uint32_t* __restrict__ cand,
                                                         uint64_t cap) {
  zs_cand_scan<EMIT>(stile, n, tcount, cand, cap, [&](uint32_t s, uint64_t u, int64_t& q0) {
    return zs_members_unit(in + in_off[s], in_len[s], u, q0);
  });
}
template __global__ void zs_k_members_scan<false>(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                                                  uint32_t, uint64_t*, uint32_t*, uint64_t);
template __global__ void zs_k_members_scan<true>(const uint8_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                                                 uint32_t, uint64_t*, uint32_t*, uint64_t);

// Lane x of the launch (zs_cand_lookup): stream x's offset 0 or candidate x - n, bounded by zs_cand_bound.
// tpre's last value is the candidates' count C (more than `cap`: the list is not complete and nothing runs).
// ZS_SYNC_LANES lanes to a workgroup, their tables in LDS, as zs_k_sync_size.
__global__ __launch_bounds__(ZS_SYNC_LANES) void zs_k_members_size(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len,
    const uint32_t* __restrict__ stile, uint32_t n, const uint64_t* __restrict__ tpre,
    const uint32_t* __restrict__ cand, uint64_t cap, uint32_t pass, zs_sync_rec* __restrict__ rec) {
  __shared__ zs_sync_tabs tabs[ZS_SYNC_LANES];
  const uint64_t x = (uint64_t)blockIdx.x * ZS_SYNC_LANES + threadIdx.x;
  const uint64_t C = tpre[stile[n]];
  if (C > cap || x >= n + C) return;
  const zs_cand_lane l = zs_cand_lookup(x, n, stile, tpre);
  const uint32_t s = l.s, start = l.k == ZS_CAND_FIRST ? 0u : cand[l.k];
  const uint32_t bound = zs_cand_bound(l, stile, tpre, cand, pass, in_len[s]);
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
