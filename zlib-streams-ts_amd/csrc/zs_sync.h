// zs_sync.h -- the two per-lane pieces of the restart-point search (inflate_sync.hip, DESIGN 4.13;
// inflateSync / syncsearch, inflate.ts:1267-1337): the candidate rule of the scan over one 16-byte
// unit, and the count-only decode from one start.  Plain C++ on the lane reader but for the funnel
// shift, so the host stand-in of tools/sync_host compiles both from this source.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_plan.h"  // zs_sync_rec, ZS_SYNC_*
#include "zs_lane_reader.h"

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

// ---- the count-only decode.  Per-lane Huffman state (LDS on the device): the symbols by (length,
// symbol) rank and the codes per length, RFC 1951 3.2.2; direct root tables for the codes of at most 9
// (literal/length) and 6 (distance) bits, u16 entries length << 12 | symbol, 0 = a longer code or none, so
// most codes cost one LDS read and only the long ones the select chain of zs_sync_decode (as the lane
// decoder's root instances, inflate_lane.hip).  541 dwords: an odd stride, so a wave's lanes fall on
// different banks.
#define ZS_SYNC_LROOT 9u
#define ZS_SYNC_DROOT 6u
struct zs_sync_tabs {
  uint16_t lsym[288];
  uint16_t lcnt[16];
  uint16_t offs[16];
  uint8_t dsym[32];  // (the header's code-length code first)
  uint8_t dcnt[16];
  uint8_t lens[320];
  uint16_t lroot[1u << ZS_SYNC_LROOT];
  uint16_t droot[1u << ZS_SYNC_DROOT];
  uint32_t pad;
};

// the code of lens[0..n): cnt[1..15], sym by rank.  Returns false when zlib's inflate_table refuses the
// set (inftrees.ts:128-139): over-subscribed, or incomplete unless it is a lone code of length 1 (never for
// the code-length code, `codes`); a set without any code builds, and no symbol decodes from it.
template <class CT, class ST>
static __device__ bool zs_sync_build(CT* cnt, ST* sym, uint16_t* offs, const uint8_t* lens, uint32_t n, bool codes) {
  for (uint32_t l = 0; l < 16u; l++) cnt[l] = 0;
  for (uint32_t i = 0; i < n; i++) cnt[lens[i] & 15u]++;
  int left = 1;
  uint32_t maxl = 0, at = 0;
  for (uint32_t l = 1; l <= 15u; l++) {
    const uint32_t c = cnt[l];
    left = 2 * left - (int)c;
    if (left < 0) return false;
    if (c) maxl = l;
    offs[l] = (uint16_t)at;
    at += c;
  }
  cnt[0] = 0;
  if (left > 0 && maxl != 0 && (codes || maxl != 1u)) return false;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = lens[i] & 15u;
    if (l) sym[offs[l]++] = (ST)i;
  }
  return true;
}

// root[x] for every code of at most `bits` bits, x the next input bits (a code travels MSB first, so
// its bits are reversed in x); after zs_sync_build: cnt[l] codes of length l, sym by rank
template <class CT, class ST>
static __device__ void zs_sync_root(uint16_t* root, uint32_t bits, const CT* cnt, const ST* sym) {
  for (uint32_t x = 0; x < (1u << bits); x++) root[x] = 0;
  uint32_t code = 0, k = 0;
  for (uint32_t l = 1; l <= bits; l++) {
    for (const uint32_t e = k + cnt[l]; k < e; k++, code++) {
      const uint32_t r = __builtin_bitreverse32(code) >> (32u - l);
      for (uint32_t x = r; x < (1u << bits); x += 1u << l) root[x] = (uint16_t)((l << 12) | (uint32_t)sym[k]);
    }
    code <<= 1;
  }
}

// the symbol at the front of the bit buffer (R.bits >= 15 or the input's end); L: its code's length, 16: none
// cnt: the codes per length in registers (zs_sync_counts), so the only memory access is the symbol's;
// selects, no branches: the lanes of a wave stand at different codes
template <class ST>
static __device__ __forceinline__ uint32_t zs_sync_decode(const zs_lane_reader& R, const uint32_t (&cnt)[16],
                                                          const ST* sym, uint32_t& L) {
  uint32_t buf = (uint32_t)R.hold, code = 0, first = 0, index = 0, at = 0, len = 16;
#pragma unroll
  for (uint32_t l = 1; l <= 15u; l++) {
    code |= buf & 1u;
    buf >>= 1;
    const uint32_t c = cnt[l];
    const bool hit = len == 16u && code < first + c;
    at = hit ? index + (code - first) : at;
    len = hit ? l : len;
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  L = len;
  return len < 16u ? (uint32_t)sym[at] : 0u;
}
template <class CT>
static __device__ __forceinline__ void zs_sync_counts(const CT* cnt, uint32_t (&r)[16]) {
#pragma unroll
  for (uint32_t l = 0; l < 16u; l++) r[l] = cnt[l];
}

// (re)start the reader at byte `at` of its input
static __device__ __forceinline__ void zs_sync_seek(zs_lane_reader& R, uint32_t at) {
  zs_lr_rewind(R, at & ~3u);
  zs_lr_fill(R);
  zs_lr_drop(R, 8u * (at & 3u));
}

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
  zs_sync_seek(R, start);
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
      zs_sync_seek(R, (uint32_t)p);
    } else if (type == 3) {
      return r;  // "invalid block type"
    } else {
      uint32_t nlen = 288, ndist = 32;
      if (type == 1) {
        for (uint32_t i = 0; i < 320u; i++) T.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
      } else {
        nlen = zs_lr_take(R, 5) + 257;
        ndist = zs_lr_take(R, 5) + 1;
        const uint32_t ncode = zs_lr_take(R, 4) + 4;
        if (nlen > 286 || ndist > 30) return r;
        uint32_t i;
        for (i = 0; i < 19u; i++) T.lens[i] = 0;
        for (i = 0; i < ncode; i++) T.lens[ZS_BL_ORDER[i]] = (uint8_t)zs_lr_take(R, 3);
        if (!zs_sync_build(T.dcnt, T.dsym, T.offs, T.lens, 19, true)) return r;
        uint32_t cc[16];
        zs_sync_counts(T.dcnt, cc);
        i = 0;
        uint32_t prev = 0;
        while (i < nlen + ndist) {
          if (R.bits < 32) zs_lr_fill(R);
          uint32_t L;
          const uint32_t v = zs_sync_decode(R, cc, T.dsym, L);
          if (L > 15) return r;
          zs_lr_drop(R, L);
          if (v < 16) {
            T.lens[i++] = (uint8_t)v;
            prev = v;
            continue;
          }
          uint32_t rep, val = 0;
          if (v == 16) {
            if (i == 0) return r;
            val = prev;
            rep = 3 + zs_lr_take(R, 2);
          } else if (v == 17) {
            rep = 3 + zs_lr_take(R, 3);
          } else {
            rep = 11 + zs_lr_take(R, 7);
          }
          if (i + rep > nlen + ndist) return r;
          while (rep--) T.lens[i++] = (uint8_t)val;
          prev = val;
        }
        if (zs_lr_bitpos(R) > limit) break;
        if (T.lens[256] == 0) return r;  // "missing end-of-block"
      }
      if (!zs_sync_build(T.lcnt, T.lsym, T.offs, T.lens, nlen, false)) return r;
      if (!zs_sync_build(T.dcnt, T.dsym, T.offs, T.lens + nlen, ndist, false)) return r;
      zs_sync_root(T.lroot, ZS_SYNC_LROOT, T.lcnt, T.lsym);
      zs_sync_root(T.droot, ZS_SYNC_DROOT, T.dcnt, T.dsym);
      uint32_t lc[16], dc[16];
      zs_sync_counts(T.lcnt, lc);
      zs_sync_counts(T.dcnt, dc);
      for (;;) {
        if (zs_lr_bitpos(R) > limit) break;
        if (R.bits < 32) zs_lr_fill(R);
        uint32_t L, sym;
        const uint32_t le = T.lroot[(uint32_t)R.hold & ((1u << ZS_SYNC_LROOT) - 1u)];
        if (le) {
          L = le >> 12;
          sym = le & 0xfffu;
        } else {
          sym = zs_sync_decode(R, lc, T.lsym, L);
          if (L > 15) return r;  // "invalid literal/length code"
        }
        zs_lr_drop(R, L);
        if (sym < 256) {
          total++;
          continue;
        }
        if (sym == 256) break;
        if (sym >= 286) return r;
        const uint32_t c = sym - 257;  // length codes: base / extra bits (inflate/constants.ts:8-23)
        uint32_t len;
        if (c < 8) {
          len = c + 3;
        } else if (c == 28) {
          len = 258;
        } else {
          const uint32_t x = (c >> 2) - 1;
          len = ((4u | (c & 3u)) << x) + 3u + zs_lr_take(R, x);
        }
        if (R.bits < 32) zs_lr_fill(R);
        uint32_t d;
        const uint32_t de = T.droot[(uint32_t)R.hold & ((1u << ZS_SYNC_DROOT) - 1u)];
        if (de) {
          L = de >> 12;
          d = de & 0xfffu;
        } else {
          d = zs_sync_decode(R, dc, T.dsym, L);
          if (L > 15) return r;  // "invalid distance code"
        }
        zs_lr_drop(R, L);
        if (d >= 30) return r;
        uint32_t dist;
        if (d < 4) {
          dist = d + 1;
        } else {
          const uint32_t x = (d >> 1) - 1;
          dist = ((2u | (d & 1u)) << x) + 1u + zs_lr_take(R, x);
        }
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
