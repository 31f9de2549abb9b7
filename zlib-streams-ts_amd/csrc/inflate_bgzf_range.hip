// inflate_bgzf_range.hip -- BGZF ranges by virtual offset (the SAM specification, section 4.1.1).
// The blocks a range touches are planned on the host from their headers (zs_plan_bgzf_range) and decode whole,
// as the members of one gzip batch, into 4-aligned staging regions.
//   zs_k_bgzf_range_end     per stream, in front of the search: where the block at the range's end ends, so that
//                           the slice the search reads stops there
//   zs_k_bgzf_range_stitch  per stream: the verdict the plan reached from the headers, or the first member
//                           that did not end cleanly; the stream's status, lengths and the length its check
//                           value is taken over
//   zs_k_bgzf_range_place   the members' delivered bytes -- without the head of a range's first block and the
//                           tail of its last -- from staging to their places; it runs behind the stitch and
//                           moves nothing that lies behind the stream's delivered length
// Every member owns its bytes of the staging buffer and of the output: no atomics, no waits between workgroups.
#include "zs_kernels.h"
#include "zs_inflate.h"
#include "zs_bgzf.h"

// One thread per stream, in front of the search: where the block at the range's end ends in the stream's slice
// (slice i: sl_len[i] bytes at in + sl_off[i]; the block starts at rce[i]), from its header where that can be
// trusted in the slice as it stands; 0 where it cannot, or where no block is needed there (rce[i] == sl_len[i]).
// The caller cuts the slice at that end: the blocks behind it -- the last of them cut short by the slice's end,
// which no header can size -- are then never scanned nor sized.
__global__ __launch_bounds__(256) void zs_k_bgzf_range_end(const uint8_t* __restrict__ in,
                                                           const uint64_t* __restrict__ sl_off,
                                                           const uint32_t* __restrict__ sl_len,
                                                           const uint32_t* __restrict__ rce, uint32_t n,
                                                           uint32_t* __restrict__ end) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t e = 0, isize = 0;
  const bool t = rce[i] < sl_len[i] && zs_bgzf_header(in + sl_off[i], sl_len[i], rce[i], e, isize);
  end[i] = t ? e : 0u;
}

// One wave per stream, zs_k_members_stitch's search: a lane per member finds the first member that did not end
// with Z_STREAM_END, a round of 64 at a time.  Lane 0 then writes the stream's fields.
//   verdict CHAIN    Z_DATA_ERROR, ZS_PHASE_PROCESS, ZS_MSG_BGZF_RANGE, out_len 0, consumed = vcons[s]
//   verdict EMPTY    Z_STREAM_END, ZS_PHASE_NONE, nothing delivered, consumed = vcons[s]
//   all members ended: Z_STREAM_END, the last member's phase and message, out_len = the delivered total,
//                    consumed = the offset behind the last member's trailer
//   else             the failing member's status, phase and message, with zs_k_members_stitch's mapping for a
//                    trusted member that outgrew its ISIZE; out_len = the delivered bytes of the members
//                    before it, consumed = its start
// cklen[s]: the delivered length, or 0 for a stream that failed.
__global__ __launch_bounds__(64) void zs_k_bgzf_range_stitch(
    const uint32_t* __restrict__ rfirst, const uint32_t* __restrict__ soff, const uint32_t* __restrict__ opos,
    const uint32_t* __restrict__ take, const uint32_t* __restrict__ verdict, const uint32_t* __restrict__ vcons,
    const int32_t* __restrict__ seg_status, const int32_t* __restrict__ seg_phase, const int32_t* __restrict__ seg_msg,
    const uint32_t* __restrict__ seg_used, uint32_t n, int32_t* __restrict__ status, int32_t* __restrict__ phase,
    int32_t* __restrict__ msg, uint32_t* __restrict__ out_len, uint32_t* __restrict__ consumed,
    uint32_t* __restrict__ cklen, const uint8_t* __restrict__ trusted) {
  const uint32_t s = blockIdx.x;
  if (s >= n) return;
  const uint32_t v = verdict[s];
  if (v != ZS_BGZF_RANGE_MEMBERS) {
    if (threadIdx.x != 0) return;
    const bool empty = v == ZS_BGZF_RANGE_EMPTY;
    status[s] = empty ? ZS_Z_STREAM_END : ZS_Z_DATA_ERROR;
    phase[s] = empty ? 0 : ZS_PHASE_PROCESS_;  // (ZS_PHASE_NONE, as every clean end)
    msg[s] = empty ? ZS_MSG_NONE : ZS_MSG_BGZF_RANGE;
    out_len[s] = 0u;
    consumed[s] = vcons[s];
    cklen[s] = 0u;
    return;
  }
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
  const bool lied = trusted[g] && seg_status[g] == ZS_Z_BUF_ERROR && seg_msg[g] == ZS_MSG_CAPACITY;
  status[s] = lied ? ZS_Z_DATA_ERROR : seg_status[g];
  phase[s] = lied ? ZS_PHASE_PROCESS_ : seg_phase[g];
  msg[s] = lied ? ZS_MSG_LENGTH_CHECK : seg_msg[g];
  // (a member that ended cleanly in its ISIZE bytes of room produced exactly those: its trailer was verified)
  out_len[s] = ok ? opos[g] + take[g] : opos[g];
  consumed[s] = ok ? soff[g] + seg_used[g] : soff[g];
  cklen[s] = ok ? opos[g] + take[g] : 0u;
}

// the segment that holds tile t: the last g with tile[g] <= t (tile: M + 1 prefix sums, tile[M] > t)
static __device__ __forceinline__ uint32_t zs_bgzf_range_find(const uint32_t* __restrict__ tile, uint32_t M, uint32_t t) {
  uint32_t lo = 0, hi = M;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tile[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// zs_k_restart_place's tiling and store rule with a source skip and a clipped length.  Member g produced
// seg_len[g] bytes (at most ocap[g]) in its staging region at stoff[g], a multiple of 4; the bytes
// [skip[g], skip[g] + L), L = min(take[g], max(produced - skip[g], 0)), go to out + dst[g], any alignment.
// Nothing moves unless the member lies inside its stream's delivered length (out_len, the stitch's): a member
// at or behind the first failure of its stream delivers nothing.  A thread owns one aligned destination word:
// a whole word is built from the one or two aligned staging words that hold its four bytes, the first and last
// partial words are stored byte by byte, each byte taken from the aligned staging word that holds it -- so a
// neighbour's bytes in the same destination word are never written, and no staging word is read that holds no
// byte of [skip, skip + L).
__global__ __launch_bounds__(256) void zs_k_bgzf_range_place(
    const uint8_t* __restrict__ stage, const uint64_t* __restrict__ stoff, const uint32_t* __restrict__ ocap,
    const uint32_t* __restrict__ seg_len, const uint32_t* __restrict__ skip, const uint32_t* __restrict__ take,
    const uint32_t* __restrict__ opos, const uint32_t* __restrict__ rstream, const uint32_t* __restrict__ out_len,
    const uint64_t* __restrict__ dst, const uint32_t* __restrict__ ptile, uint32_t M, uint8_t* __restrict__ out) {
  const uint32_t T = ptile[M];
  for (uint32_t t = blockIdx.x; t < T; t += gridDim.x) {
    const uint32_t g = zs_bgzf_range_find(ptile, M, t);
    const uint32_t made = min(seg_len[g], ocap[g]), sk = skip[g];
    const uint32_t L = min(take[g], made > sk ? made - sk : 0u);
    if (L == 0 || (uint64_t)opos[g] + L > out_len[rstream[g]]) continue;
    const uint64_t d0 = dst[g];
    const uint32_t head = (uint32_t)(d0 & 3u);  // the destination's offset in its first word
    const uint64_t words = ((uint64_t)head + L + 3u) >> 2;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(stage + stoff[g]);
    uint8_t* o = out + (d0 - head);
    const uint64_t w0 = (uint64_t)(t - ptile[g]) * (ZS_RESTART_TILE / 4u);
    for (uint32_t k = threadIdx.x; k < ZS_RESTART_TILE / 4u; k += 256u) {
      const uint64_t w = w0 + k;
      if (w >= words) break;
      const uint64_t lo = 4u * w, hi = lo + 4u;  // this word's bytes, relative to the first word's start
      if (lo >= head && hi <= (uint64_t)head + L) {
        const uint32_t b = sk + (uint32_t)(lo - head);  // the staging byte of the word's first byte
        const uint32_t sh = b & 3u;
        uint32_t v = sw[b >> 2];
        if (sh) v = __builtin_amdgcn_alignbyte(sw[(b >> 2) + 1u], v, sh);  // (holds byte b + 3 < skip + L)
        *reinterpret_cast<uint32_t*>(o + lo) = v;
      } else {
        for (uint64_t at = lo < head ? head : lo; at < hi && at < (uint64_t)head + L; at++) {
          const uint32_t b = sk + (uint32_t)(at - head);
          o[at] = (uint8_t)(sw[b >> 2] >> (8u * (b & 3u)));
        }
      }
    }
  }
}
