// zs_members.h -- the two per-lane pieces of the search for a gzip file's members (inflate_members.hip,
// DESIGN 4.14; zlib's gz_look, gzread.c): the candidate rule of the scan over one 16-byte unit, and
// the sizing of one member from its start -- the header's parse, the count-only decode of zs_sync.h
// to the final block, the trailer's eight bytes.  Plain C++ but for the funnel shift, so the host
// stand-in of tools/members_host compiles both from this source.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_sync.h"

// ---- the scan.  A stream's bytes s[0..n) lie in the 16-byte units that start at s - ((uintptr_t)s & 15);
// unit u's byte i is the stream's byte q0 + i, q0 = 16 u - sh16.  A candidate is an offset q >= 1 with
// q + 4 <= n whose four bytes pass zs_member_magic: 1f 8b 08, then a flag byte without a reserved bit.
// Returns unit u's mask: bit i set when q0 + i is a candidate.  Only aligned words that hold bytes of
// the stream are loaded (the word behind the unit too: the pattern may straddle words, units and tiles).
static __device__ __forceinline__ uint32_t zs_members_unit(const uint8_t* s, uint32_t n, uint64_t u, int64_t& q0) {
  const uint32_t sh16 = (uint32_t)((uintptr_t)s & 15u);
  const uint32_t* base = reinterpret_cast<const uint32_t*>(s - sh16);
  q0 = (int64_t)(16u * u) - (int64_t)sh16;
  if (n == 0 || 16u * u >= (uint64_t)sh16 + n) return 0u;
  const uint64_t wlo = sh16 >> 2, whi = ((uint64_t)sh16 + n - 1u) >> 2;  // the words that hold the stream's bytes
  const uint64_t k0 = 4u * u;
  uint32_t w[5];
  if (k0 >= wlo && k0 + 3u <= whi) {
    const uint4 v = *reinterpret_cast<const uint4*>(base + k0);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) w[k] = (k0 + k >= wlo && k0 + k <= whi) ? base[k0 + k] : 0u;
  }
  w[4] = (k0 + 4u <= whi) ? base[k0 + 4u] : 0u;  // (k0 + 4 > wlo as the unit holds a byte of the stream)
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t i = 0; i < 16u; i++) {
    // the four bytes that start with the unit's byte i: bytes i .. i + 3 of w[0..4]
    const uint32_t a = i >> 2, sh = i & 3u;
    const uint32_t v = sh ? __builtin_amdgcn_alignbyte(w[a + 1], w[a], sh) : w[a];
    const int64_t q = q0 + (int64_t)i;
    if ((v & 0xe0ffffffu) == 0x00088b1fu && q >= 1 && q + 4 <= (int64_t)n) mask |= 1u << i;
  }
  return mask;
}

// ---- one member sized.  One lane: the gzip member of s[0..n) that starts at byte `start`, its header
// parsed by zs_wrapper_header_len_of's rules, its deflate blocks counted and not stored to the final
// block without stopping at markers, its trailer's eight bytes required (the decoder verifies them).
// The lane reads no byte at or past `bound` (<= n).  The ends:
//   the header, the data or the trailer pass the bound   ZS_SYNC_PASSED (bound < n) or ZS_SYNC_ERROR (the
//                                                        input is exhausted)
//   the four bytes at `start` are no member's, the deflate data is invalid, a copy reaches before the
//   member's start, more than 2^32 - 1 bytes produced    ZS_SYNC_ERROR
//   else                                                 ZS_SYNC_FINAL, end = the offset behind the trailer,
//                                                        len = the bytes produced
static __device__ zs_sync_rec zs_members_size(const uint8_t* s, uint32_t n, uint32_t start, uint32_t bound,
                                              zs_sync_tabs& T) {
  zs_sync_rec r = {ZS_SYNC_ERROR, start, 0u, 0u};
  const uint32_t out_of_input = bound < n ? ZS_SYNC_PASSED : ZS_SYNC_ERROR;
  if (start >= bound || bound - start < 4u) {
    r.how = out_of_input;
    return r;
  }
  if (!zs_member_magic(s + start)) return r;
  const uint32_t hl = zs_wrapper_header_len_of(31, s + start, bound - start);
  if (hl == 0) {  // (the magic holds: the header does not end in front of the bound)
    r.how = out_of_input;
    return r;
  }
  const zs_sync_rec d = zs_sync_size(s, n, start + hl, bound, T, true);
  r.end = d.end;
  r.len = d.len;
  if (d.how != ZS_SYNC_FINAL) {
    r.how = d.how;
    return r;
  }
  if (d.reach) return r;
  if ((uint64_t)d.end + 8u > bound) {
    r.how = out_of_input;
    return r;
  }
  r.how = ZS_SYNC_FINAL;
  r.end = d.end + 8u;
  return r;
}
