// zs_sync.h -- the two per-lane pieces of the restart-point search (inflate_sync.hip, DESIGN 4.13;
// inflateSync / syncsearch, inflate.ts:1267-1337): the candidate rule of the scan over one 16-byte
// unit, and the count-only decode from one start, on the lane reader and the per-lane Huffman code
// of zs_lane_huff.h.  Plain C++ but for the funnel shift, so the host stand-in of tools/sync_host
// compiles both from this source.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_plan.h"  // zs_sync_rec, ZS_SYNC_*
#include "zs_inftab.h"  // zs_lbase, zs_dbase
#include "zs_lane_huff.h"

// ---- the scan.  A stream's bytes s[0..n) lie in the 16-byte units that start at s - ((uintptr_t)s & 15);
// unit u's byte i is the stream's byte 16 u + i - sh16.  A candidate is an offset q with
// s[q-4..q) == 00 00 FF FF, first + 4 <= q <= n.  Returns unit u's mask: bit i set when the marker's
// last byte is the unit's byte i, i.e. q = q0 + i.  Only aligned words that hold bytes of the stream
// are loaded (the word in front of the unit too: a marker may straddle units, tiles and words).
static __device__ __forceinline__ uint32_t zs_sync_unit(const uint8_t* s, uint32_t n, uint32_t first, uint64_t u,
                                                        int64_t& q0) {
  const uint32_t sh16 = (uint32_t)((uintptr_t)s & 15u);
  const uint32_t* base = reinterpret_cast<const uint32_t*>(s - sh16);
  q0 = (int64_t)(16u * u) + 1 - (int64_t)sh16;
  if (n == 0 || 16u * u >= (uint64_t)sh16 + n) return 0u;
  const uint64_t wlo = sh16 >> 2, whi = ((uint64_t)sh16 + n - 1u) >> 2;  // the words that hold the stream's bytes
  const uint64_t k0 = 4u * u;
  uint32_t w[5];
  w[0] = (k0 > wlo) ? base[k0 - 1u] : 0u;  // (k0 - 1 >= wlo; k0 - 1 <= whi as the unit holds a byte of the stream)
  if (k0 >= wlo && k0 + 3u <= whi) {
    const uint4 v = *reinterpret_cast<const uint4*>(base + k0);
    w[1] = v.x;
    w[2] = v.y;
    w[3] = v.z;
    w[4] = v.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) w[k + 1] = (k0 + k >= wlo && k0 + k <= whi) ? base[k0 + k] : 0u;
  }
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t i = 0; i < 16u; i++) {
    // the four bytes that end with the unit's byte i: bytes i + 1 .. i + 4 of w[0..4]
    const uint32_t a = (i + 1u) >> 2, sh = (i + 1u) & 3u;
    const uint32_t v = sh ? __builtin_amdgcn_alignbyte(w[a + 1], w[a], sh) : w[a];
    const int64_t q = q0 + (int64_t)i;
    if (v == 0xffff0000u && q >= (int64_t)first + 4 && q <= (int64_t)n) mask |= 1u << i;
  }
  return mask;
}

// ---- the count-only decode.  A lane's tables (LDS on the device) for zs_lane_huff.h's code: the
// symbols by rank, the build's counts, the block's code lengths, and direct root tables for the codes
// of at most 9 (literal/length) and 6 (distance) bits, as the lane decoder's root instances keep
// them.  The codes' limits (zs_canon) stay in registers: one wave to a SIMD has them to spare, and
// LDS is what bounds the workgroups of a CU.  537 dwords: an odd stride, so a wave's lanes fall on
// different banks.
#define ZS_SYNC_DROOT 6u
struct zs_sync_tabs {
  uint32_t cnt[16];
  uint16_t lsym[288];
  uint8_t dsym[32];  // (the header's code-length code first)
  uint8_t lens[320];
  uint16_t lroot[1u << ZS_LROOT];
  uint16_t droot[1u << ZS_SYNC_DROOT];
  uint32_t pad;
};

// One lane: the deflate blocks of s[0..n) from byte `start` on, counted and not stored, no history read.
// The lane reads no byte at or past `bound` (<= n): its reader ends there and returns zeros, and the
// bit position is checked against it before every block and every symbol.  The ends, in this order:
//   past the bound                       ZS_SYNC_PASSED (bound < n) or ZS_SYNC_ERROR (the input is exhausted)
//   an invalid block type, stored lengths, code set or code, a distance symbol that does not exist,
//   more than 2^32 - 1 bytes produced     ZS_SYNC_ERROR
//   the final block closed                ZS_SYNC_FINAL, end = the bytes consumed
//   a block closed at a byte boundary q >= start + 5 with s[q-4..q) == 00 00 FF FF
//                                         ZS_SYNC_LANDED, end = q
// len: the bytes produced up to `end`; reach: the largest distance - bytes produced so far over the
// copies, 0 when none is positive (a copy from before the start).
// to_end: the lane does not stop where it lands (the reach of a whole tail, zs_k_sync_tail).
static __device__ zs_sync_rec zs_sync_size(const uint8_t* s, uint32_t n, uint32_t start, uint32_t bound,
                                           zs_sync_tabs& T, bool to_end = false) {
  zs_sync_rec r = {ZS_SYNC_ERROR, start, 0u, 0u};
  const uint32_t out_of_input = bound < n ? ZS_SYNC_PASSED : ZS_SYNC_ERROR;
  if (start >= bound) {
    r.how = out_of_input;
    return r;
  }
  zs_lane_reader R;
  zs_lr_init(R, s, bound);
  zs_lr_seek(R, 8ull * start);
  const uint64_t limit = (uint64_t)bound * 8u;
  uint64_t total = 0;
  uint32_t& reach = r.reach;  // (current at every return)
  for (;;) {
    if (zs_lr_bitpos(R) > limit) break;
    const bool last = zs_lr_take(R, 1) != 0;
    const uint32_t type = zs_lr_take(R, 2);
    if (type == 0) {  // stored: skipped, not copied
      zs_lr_align(R);
      const uint32_t len = zs_lr_take(R, 16), nlen = zs_lr_take(R, 16);
      if (zs_lr_bitpos(R) > limit) break;
      if (len != (nlen ^ 0xffffu)) return r;
      const uint64_t p = (zs_lr_bitpos(R) >> 3) + len;
      if (p > bound) break;
      total += len;
      zs_lr_seek(R, 8u * p);
    } else if (type == 3) {
      return r;  // "invalid block type"
    } else {
      uint32_t nlen = 288, ndist = 32;
      zs_canon CL, CD;
      if (type == 1) {
        zs_lane_fixed_lengths(T.lens);
      } else {
        if (!zs_lane_code_lengths<false>(R, false, CD, T.cnt, T.dsym, T.lens, nlen, ndist)) return r;
        if (zs_lr_bitpos(R) > limit) break;
      }
      // (zlib decodes with an incomplete set it takes, ZS_CODE_PARTIAL: a code it lacks ends the lane)
      if (zs_canon_build(CL, T.cnt, T.lsym, nullptr, T.lens, nlen, false) == ZS_CODE_REFUSED) return r;
      zs_root_fill(T.lroot, ZS_LROOT, CL, T.cnt, T.lsym, nullptr);
      if (zs_canon_build(CD, T.cnt, T.dsym, nullptr, T.lens + nlen, ndist, false) == ZS_CODE_REFUSED) return r;
      zs_root_fill(T.droot, ZS_SYNC_DROOT, CD, T.cnt, T.dsym, nullptr);
      for (;;) {
        if (zs_lr_bitpos(R) > limit) break;
        if (R.bits < 32) zs_lr_fill(R);
        uint32_t L, sym;
        const uint32_t le = T.lroot[(uint32_t)R.hold & ((1u << ZS_LROOT) - 1u)];
        if (le) {
          L = le >> 12;
          sym = le & 0xfffu;
        } else {
          const uint32_t k = zs_canon_rank(CL, R, L);
          if (L > 15) return r;  // "invalid literal/length code"
          sym = T.lsym[k];
        }
        zs_lr_drop(R, L);
        if (sym < 256) {
          total++;
          continue;
        }
        if (sym == 256) break;
        if (sym >= 286) return r;
        uint32_t base, op;
        zs_lbase(sym - 257, false, base, op);
        const uint32_t len = base + zs_lr_take(R, op & 15u);
        if (R.bits < 32) zs_lr_fill(R);
        uint32_t d;
        const uint32_t de = T.droot[(uint32_t)R.hold & ((1u << ZS_SYNC_DROOT) - 1u)];
        if (de) {
          L = de >> 12;
          d = de & 0xfffu;
        } else {
          const uint32_t k = zs_canon_rank(CD, R, L);
          if (L > 15) return r;  // "invalid distance code"
          d = T.dsym[k];
        }
        zs_lr_drop(R, L);
        if (d >= 30) return r;
        zs_dbase(d, false, base, op);
        const uint32_t dist = base + zs_lr_take(R, op & 15u);
        if (dist > total && dist - total > reach) reach = (uint32_t)(dist - total);
        total += len;
      }
    }
    // a block has closed
    const uint64_t bit = zs_lr_bitpos(R);
    if (bit > limit) break;
    if (total > 0xffffffffull) return r;
    r.len = (uint32_t)total;
    if (last) {
      r.how = ZS_SYNC_FINAL;
      r.end = (uint32_t)((bit + 7u) >> 3);
      return r;
    }
    if ((bit & 7u) == 0 && !to_end) {
      const uint32_t q = (uint32_t)(bit >> 3);
      if ((uint64_t)q >= (uint64_t)start + ZS_RESTART_MIN_GAP && s[q - 4] == 0 && s[q - 3] == 0 && s[q - 2] == 0xff && s[q - 1] == 0xff) {
        r.how = ZS_SYNC_LANDED;
        r.end = q;
        return r;
      }
    }
  }
  // past the bound: the record is what the last closed block left
  r.how = out_of_input;
  r.len = total > 0xffffffffull ? 0xffffffffu : (uint32_t)total;
  r.end = bound;
  return r;
}
