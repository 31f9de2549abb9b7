// inflate_restart.hip -- a stream decoded from its restart points (inflateSync,
// inflate.ts:1267-1337: behind 00 00 FF FF the reference resets the stream, the window with it).
//
// A stream that comes with k points is k SEGMENTS (zs_plan_restart).  Every segment but a stream's last
// ends with the marker's empty stored block, BFINAL clear, which no decoder here takes for a clean
// end; so the segments are copied and the copies closed:
//   zs_k_restart_gather   the segments into the gather buffer, each at a multiple of 16 bytes, 03 00
//                         (the empty final static block) behind every one that is not its stream's
//                         last, zeros to the next multiple of 16; whether a segment's last four source
//                         bytes are the marker
//   (the copies decode as the members of one raw batch, by the decoders as they are)
//   zs_k_restart_place    staging route only (a restart out_pos that is no multiple of 4): the
//                         segments' bytes from their 4-aligned staging regions to their places
//   zs_k_restart_stitch   per stream: the first segment that fails its conditions, the header, the
//                         trailer; the stream's status, lengths and expected check value
//   zs_k_restart_check    after the data checksum over the joined output: the check value, or the failure
// Every segment owns its bytes of the gather buffer and of the output: no atomics, no waits between
// workgroups.
#include "zs_kernels.h"
#include "zs_inflate.h"

// the segment that holds tile t: the last g with tile[g] <= t (tile: M + 1 prefix sums, tile[M] > t)
static __device__ __forceinline__ uint32_t zs_restart_find(const uint32_t* __restrict__ tile, uint32_t M, uint32_t t) {
  uint32_t lo = 0, hi = M;  // tile[lo] <= t < tile[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tile[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// 16 source bytes from p (any alignment, all 16 inside the segment): aligned words and funnel shifts
static __device__ __forceinline__ uint4 zs_restart_load16(const uint8_t* p) {
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p - sh);
  if (sh == 0) {
    if (((uintptr_t)p & 15u) == 0) return *reinterpret_cast<const uint4*>(p);
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
  const uint32_t a = w[0], b = w[1], c = w[2], d = w[3], e = w[4];  // (w[4] holds byte 15: inside the segment)
  return make_uint4(__builtin_amdgcn_alignbyte(b, a, sh), __builtin_amdgcn_alignbyte(c, b, sh),
                    __builtin_amdgcn_alignbyte(d, c, sh), __builtin_amdgcn_alignbyte(e, d, sh));
}

// One workgroup step copies ZS_RESTART_TILE bytes of one segment's copy, 16 per lane; the grid strides
// over the call's tiles, so a 300-byte segment takes one step and a 1 MiB segment 256 of them.
// src[g]: the segment's first byte in `in`; slen / glen: its source length / its copy's (slen, or slen +
// 2 for 03 00); goff[g]: the copy's place, a multiple of 16; the copy is written to the next multiple of
// 16 past glen.  mark[g] = 1 when the last four source bytes are 00 00 FF FF (and for a stream's last
// segment, which ends by itself).  `in` is only read.
__global__ __launch_bounds__(256) void zs_k_restart_gather(const uint8_t* __restrict__ in,
                                                           const uint64_t* __restrict__ src,
                                                           const uint32_t* __restrict__ slen,
                                                           const uint32_t* __restrict__ glen,
                                                           const uint64_t* __restrict__ goff,
                                                           const uint32_t* __restrict__ gtile, uint32_t M,
                                                           uint8_t* __restrict__ gather,
                                                           uint32_t* __restrict__ mark) {
  const uint32_t T = gtile[M];
  for (uint32_t t = blockIdx.x; t < T; t += gridDim.x) {
    const uint32_t g = zs_restart_find(gtile, M, t);
    const uint32_t n = slen[g], gn = glen[g];
    const uint64_t end = ((uint64_t)gn + 15u) & ~15ull;
    const uint64_t b = (uint64_t)(t - gtile[g]) * ZS_RESTART_TILE + threadIdx.x * 16u;
    const uint8_t* s = in + src[g];
    if (t == gtile[g] && threadIdx.x == 0) {
      uint32_t m = 1;
      if (gn != n) m = n >= 4u && s[n - 4] == 0 && s[n - 3] == 0 && s[n - 2] == 0xff && s[n - 1] == 0xff;
      mark[g] = m;
    }
    if (b >= end) continue;
    uint4 v;
    if (b + 16u <= n) {
      v = zs_restart_load16(s + b);
    } else {
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t k = 0; k < 16u; k++) {
        const uint64_t at = b + k;
        // the source bytes, then 03 00 (gn == n + 2), then zeros
        const uint32_t by = at < n ? s[at] : (at == n && gn != n) ? 3u : 0u;
        w[k >> 2] |= by << (8u * (k & 3u));
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(gather + goff[g] + b) = v;
  }
}

// Staging route: segment g's produced bytes (at most its capacity) from its 4-aligned staging region
// to out + dst[g], any alignment.  A thread owns one aligned destination word: whole words are built
// from two aligned staging words, the segment's first and last partial words are stored byte by byte,
// so a neighbour's bytes in the same word are never written.
__global__ __launch_bounds__(256) void zs_k_restart_place(const uint8_t* __restrict__ stage,
                                                          const uint64_t* __restrict__ stoff,
                                                          const uint32_t* __restrict__ ocap,
                                                          const uint32_t* __restrict__ seg_len,
                                                          const uint64_t* __restrict__ dst,
                                                          const uint32_t* __restrict__ ptile, uint32_t M,
                                                          uint8_t* __restrict__ out) {
  const uint32_t T = ptile[M];
  for (uint32_t t = blockIdx.x; t < T; t += gridDim.x) {
    const uint32_t g = zs_restart_find(ptile, M, t);
    const uint32_t L = min(seg_len[g], ocap[g]);
    if (L == 0) continue;
    const uint64_t d0 = dst[g];
    const uint32_t head = (uint32_t)(d0 & 3u);  // the destination's offset in its first word
    const uint64_t words = ((uint64_t)head + L + 3u) >> 2;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(stage + stoff[g]);
    const uint8_t* sb = stage + stoff[g];
    uint8_t* o = out + (d0 - head);
    const uint32_t sh = (4u - head) & 3u;  // staging byte of a whole word's first byte, modulo 4
    const uint64_t w0 = (uint64_t)(t - ptile[g]) * (ZS_RESTART_TILE / 4u);
    for (uint32_t k = threadIdx.x; k < ZS_RESTART_TILE / 4u; k += 256u) {
      const uint64_t w = w0 + k;
      if (w >= words) break;
      const uint64_t lo = 4u * w, hi = lo + 4u;  // this word's bytes, relative to the first word's start
      if (lo >= head && hi <= (uint64_t)head + L) {
        const uint64_t sidx = (lo - head) >> 2;  // the staging word holding its first byte
        uint32_t v = sw[sidx];
        if (sh) v = __builtin_amdgcn_alignbyte(sw[sidx + 1], v, sh);  // (its last byte < L <= the region's words)
        *reinterpret_cast<uint32_t*>(o + lo) = v;
      } else {
        for (uint64_t at = lo < head ? head : lo; at < hi && at < (uint64_t)head + L; at++) o[at] = sb[at - head];
      }
    }
  }
}

// One wave per stream.  A lane per segment finds the first segment that fails its conditions, a round of
// 64 at a time with the first failure carried across rounds: every segment ended cleanly; one that is not
// the stream's last has the marker in its last four bytes, consumed its bytes and the two appended ones
// and produced exactly the bytes up to the next point.  Lane 0 then checks the header in front of the
// first point and reads the trailer behind the last segment's final block.
// The capacity outcome (the plain entry's: Z_BUF_ERROR, "output capacity exceeded") when the last
// point lies past out_cap or the last segment is the first to fail and ran out of room; any other
// failure is Z_DATA_ERROR, ZS_MSG_RESTART, all lengths 0.  want[s]: the trailer's check value.
__global__ __launch_bounds__(64) void zs_k_restart_stitch(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len,
    const uint32_t* __restrict__ over, const uint32_t* __restrict__ rfirst, const uint32_t* __restrict__ soff,
    const uint32_t* __restrict__ slen, const uint32_t* __restrict__ olen, const uint32_t* __restrict__ opos,
    const uint32_t* __restrict__ mark, const int32_t* __restrict__ seg_status, const int32_t* __restrict__ seg_msg,
    const uint32_t* __restrict__ seg_len, const uint32_t* __restrict__ seg_used, int wbits, uint32_t n,
    int32_t* __restrict__ status, int32_t* __restrict__ phase, int32_t* __restrict__ msg, uint32_t* __restrict__ out_len,
    uint32_t* __restrict__ consumed, uint32_t* __restrict__ want) {
  const uint32_t s = blockIdx.x;
  if (s >= n) return;
  const uint32_t g0 = rfirst[s], g1 = rfirst[s + 1], last = g1 - 1u;
  uint32_t bad = 0xffffffffu;
  for (uint32_t base = g0; base < g1 && bad == 0xffffffffu; base += 64u) {
    const uint32_t g = base + threadIdx.x;
    bool fails = false;
    if (g < g1) {
      fails = seg_status[g] != ZS_Z_STREAM_END;
      if (g != last) fails = fails || !mark[g] || seg_used[g] != slen[g] + 2u || seg_len[g] != olen[g];
    }
    const unsigned long long m = __ballot(fails);
    if (m) bad = base + (uint32_t)__ffsll(m) - 1u;
  }
  if (threadIdx.x != 0) return;
  int32_t st = ZS_Z_DATA_ERROR, ph = ZS_PHASE_PROCESS_, mg = ZS_MSG_RESTART;
  uint32_t ol = 0, used = 0, w = 0;
  const uint8_t* p = in + in_off[s];
  const uint32_t n_in = in_len[s];
  if (over[s] || (bad == last && seg_status[last] == ZS_Z_BUF_ERROR && seg_msg[last] == ZS_MSG_CAPACITY)) {
    st = ZS_Z_BUF_ERROR;
    ph = ZS_PHASE_NONE_;
    mg = ZS_MSG_CAPACITY;
  } else if (bad == 0xffffffffu && zs_wrapper_header_ok(wbits, p, n_in, soff[g0])) {
    const uint32_t tl = wbits == 31 ? 8u : wbits == 15 ? 4u : 0u;
    const uint64_t tp = (uint64_t)soff[last] + seg_used[last];  // behind the final block
    const uint64_t total = (uint64_t)opos[last] + seg_len[last];
    bool ok = tp + tl <= n_in && total <= 0xffffffffull;
    if (ok && wbits == 31) {  // crc32 and ISIZE, little-endian (inflate.ts:1071-1101)
      const uint8_t* t = p + tp;
      w = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
      const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
      ok = isize == (uint32_t)total;
    } else if (ok && wbits == 15) {  // adler32, big-endian (inflate.ts:1045-1069)
      const uint8_t* t = p + tp;
      w = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | (uint32_t)t[3];
    }
    if (ok) {
      st = ZS_Z_STREAM_END;
      ph = ZS_PHASE_NONE_;
      mg = ZS_MSG_NONE;
      ol = (uint32_t)total;
      used = (uint32_t)(tp + tl);
    }
  }
  status[s] = st;
  phase[s] = ph;
  msg[s] = mg;
  out_len[s] = ol;
  consumed[s] = used;
  want[s] = w;
}

// sum[s]: the data checksum over the stream's joined output (out_len[s] bytes).  A wrapped stream whose
// trailer disagrees becomes the failure; check[s] (may be null) as zs_inflate_batch_ex: the check
// value of a wrapped stream that succeeded, else 0.
__global__ void zs_k_restart_check(const uint32_t* __restrict__ sum, const uint32_t* __restrict__ want, int wbits,
                                   uint32_t n, int32_t* __restrict__ status, int32_t* __restrict__ phase,
                                   int32_t* __restrict__ msg, uint32_t* __restrict__ out_len,
                                   uint32_t* __restrict__ consumed, uint32_t* __restrict__ check) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  uint32_t v = 0;
  if (status[s] == ZS_Z_STREAM_END && wbits > 0) {
    if (sum[s] == want[s]) {
      v = sum[s];
    } else {
      status[s] = ZS_Z_DATA_ERROR;
      phase[s] = ZS_PHASE_PROCESS_;
      msg[s] = ZS_MSG_RESTART;
      out_len[s] = 0;
      consumed[s] = 0;
    }
  }
  if (check) check[s] = v;
}
