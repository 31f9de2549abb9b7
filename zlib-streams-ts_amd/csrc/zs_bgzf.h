// zs_bgzf.h -- the per-lane piece of the BGZF fast path (inflate_bgzf.hip; the SAM
// specification, section 4.1: a gzip member whose extra field holds the subfield 'B' 'C' with the
// member's size, BSIZE, and whose trailer's ISIZE is at most 65,536).  A start whose header can be
// TRUSTED is sized from three of its words -- where it ends from BSIZE, what it produces from ISIZE --
// and no deflate byte is read; every other start is sized by zs_members_size itself.  Plain C++, so the
// host stand-in of tools/bgzf_host and the host's zs_bgzf_out_len compile it from this source (the host
// layer defines ZS_BGZF_HOST_ONLY: the header's rule and the chain, without the lane and its decoder).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_plan.h"  // zs_member_magic, zs_sync_rec
#ifndef ZS_BGZF_HOST_ONLY
#include "zs_members.h"
#endif

#if defined(__HIPCC__)
#define ZS_BGZF_FN static __host__ __device__ __forceinline__
#else
#define ZS_BGZF_FN static inline
#endif

#define ZS_BGZF_ISIZE_MAX 65536u  // a block's data at most (the specification's 64 KiB)

// The stream's bytes [at, at + 4), at < n, little-endian: the two aligned words that hold them (the second
// clamped to the word of the stream's last byte: what the value holds of bytes at or past n is not the
// stream's, and the caller masks it) and a funnel shift.  Only aligned words that hold bytes of the stream
// are loaded, the rule of zs_members_unit and the lane reader.
ZS_BGZF_FN uint32_t zs_bgzf_le32(const uint8_t* s, uint32_t n, uint32_t at) {
  const uint32_t sh4 = (uint32_t)((uintptr_t)s & 3u);
  const uint32_t* w4 = reinterpret_cast<const uint32_t*>(s - sh4);
  const uint64_t b = (uint64_t)sh4 + at, q = b >> 2, last = ((uint64_t)sh4 + n - 1u) >> 2;
  const uint32_t lo = w4[q], hi = w4[q + 1u < last ? q + 1u : last];
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * ((uint32_t)b & 3u)));
}

// The header at offset p of s[0..n) is TRUSTED when
//   p + 18 <= n and s[p..p+4) is 1f 8b 08 04 (FLG exactly 4: FEXTRA alone);
//   XLEN (u16 at p + 10) has p + 12 + XLEN <= n, and the subfields SI1 SI2 SLEN data tile the XLEN bytes exactly;
//   one subfield is 'B' 'C' with SLEN 2: the first such one gives BSIZE (it need not be the first subfield);
//   total = BSIZE + 1 > 12 + XLEN + 8 (at least one byte of deflate data) and p + total <= n;
//   ISIZE (u32 at p + total - 4) <= 65,536.
// Then end = p + total, isize = ISIZE.  A BGZF writer's own header (BC first, XLEN 6) costs the four words
// at p, p + 8, p + 12 and p + 16, which do not depend on each other, and the trailer's word.
ZS_BGZF_FN bool zs_bgzf_header(const uint8_t* s, uint32_t n, uint32_t p, uint32_t& end, uint32_t& isize) {
  if ((uint64_t)p + 18u > n) return false;
  if (zs_bgzf_le32(s, n, p) != 0x04088b1fu) return false;
  const uint32_t xlen = zs_bgzf_le32(s, n, p + 8u) >> 16;
  const uint64_t x1 = (uint64_t)p + 12u + xlen;  // the offset behind the extra field
  if (x1 > n) return false;
  uint64_t at = (uint64_t)p + 12u;
  uint32_t bsize = 0;
  bool found = false;
  while (at + 4u <= x1) {
    const uint32_t h = zs_bgzf_le32(s, n, (uint32_t)at);  // SI1 SI2 SLEN
    const uint32_t slen = h >> 16;
    if (at + 4u + slen > x1) return false;
    if (!found && h == 0x00024342u) {
      bsize = zs_bgzf_le32(s, n, (uint32_t)at + 4u) & 0xffffu;  // (its two bytes lie inside the extra field)
      found = true;
    }
    at += 4u + slen;
  }
  if (at != x1 || !found) return false;
  const uint32_t total = bsize + 1u;
  if (total <= 12u + xlen + 8u || (uint64_t)p + total > n) return false;
  isize = zs_bgzf_le32(s, n, p + total - 4u);
  if (isize > ZS_BGZF_ISIZE_MAX) return false;
  end = p + total;
  return true;
}

#ifndef ZS_BGZF_HOST_ONLY
// One START sized: the trusted header's record {ZS_SYNC_FINAL, end = p + BSIZE + 1, len = ISIZE, reach = 0},
// whatever the lane's bound is (nothing between the header and the trailer is read); else zs_members_size's
// own record under the bound.  trusted: which of the two it was.
static __device__ __forceinline__ zs_sync_rec zs_bgzf_size(const uint8_t* s, uint32_t n, uint32_t start, uint32_t bound,
                                                           zs_sync_tabs& T, bool& trusted) {
  zs_sync_rec r = {ZS_SYNC_FINAL, 0u, 0u, 0u};
  trusted = zs_bgzf_header(s, n, start, r.end, r.len);
  return trusted ? r : zs_members_size(s, n, start, bound, T);
}
#endif

// Host arithmetic over a whole file (zs_bgzf_out_len): the trusted headers followed from 0 by the members'
// ending rule -- behind a block the chain goes on where the four-byte test of a member's start holds, and
// ends where it fails or the input ends.  1 and the sum of ISIZE when every member on the chain is trusted;
// 0 when the chain meets one that is not (offset 0 is a member whatever its bytes are: an empty input is 0).
ZS_BGZF_FN int zs_bgzf_chain(const uint8_t* s, uint32_t n, uint64_t& total) {
  uint32_t p = 0;
  total = 0;
  for (;;) {
    uint32_t end, isize;
    if (!zs_bgzf_header(s, n, p, end, isize)) return 0;
    total += isize;
    p = end;
    if ((uint64_t)p + 4u > n || !zs_member_magic(s + p)) return 1;
  }
}

// ---- a range by virtual offset (the SAM specification, section 4.1.1: a virtual offset is
// coffset << 16 | uoffset, coffset a block's start in the file and uoffset a position in the block's data).
// Headers are trusted inside the range's slice (zs_bgzf_range_slice, zs_plan.h): a block that passes its end
// is not.
// Host arithmetic over one range (zs_bgzf_range_out_len), by the rule zs_plan_bgzf_range applies to the
// device's records: the chain of trusted headers from cb lands on ce exactly, the block at ce is trusted when
// ue > 0, ub and ue lie inside their blocks.  1 and the delivered length; 0 where the plan fails the stream.
ZS_BGZF_FN int zs_bgzf_range_chain(const uint8_t* s, uint32_t n, uint64_t vb, uint64_t ve, uint64_t& total) {
  total = 0;
  const uint64_t cb = vb >> 16, ce = ve >> 16;
  const uint32_t ub = (uint32_t)(vb & 0xffffu), ue = (uint32_t)(ve & 0xffffu);
  if (vb > ve || ce > n) return 0;
  uint32_t off, len;
  zs_bgzf_range_slice(n, vb, ve, off, len);
  const uint8_t* z = s + off;
  const uint32_t rce = (uint32_t)(ce - cb);
  uint32_t p = 0, end, isize;
  uint64_t sum = 0;
  while (p < rce) {
    if (!zs_bgzf_header(z, len, p, end, isize) || end > rce) return 0;
    if (p == 0 && ub > isize) return 0;
    sum += isize;
    p = end;
  }
  if (ue) {
    if (!zs_bgzf_header(z, len, p, end, isize) || ue > isize) return 0;
    sum += ue;
  }
  total = sum - ub;  // (cb == ce: ub <= ue, both in the one block)
  return 1;
}

// The virtual offset of uncompressed position upos from one stream's index of (block_in, block_out), `count`
// entries in increasing order, the end entry included where present (zs_last_bgzf_blocks, zs_last_members):
// the last block with block_out <= upos.  0 when upos lies behind the last entry or in front of the first, or
// the difference does not fit 16 bits.
static inline int zs_bgzf_voffset_of(const uint32_t* block_in, const uint32_t* block_out, uint64_t count, uint64_t upos,
                                     uint64_t& voff) {
  voff = 0;
  if (!count || !block_in || !block_out || upos > block_out[count - 1] || upos < block_out[0]) return 0;
  uint64_t lo = 0, hi = count;  // block_out[lo] <= upos < block_out[hi]
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (block_out[mid] <= upos) lo = mid;
    else hi = mid;
  }
  const uint64_t d = upos - block_out[lo];
  if (d > 0xffffu) return 0;
  voff = ((uint64_t)block_in[lo] << 16) | d;
  return 1;
}
