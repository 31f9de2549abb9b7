// zs_lane_huff.h -- one lane's Huffman code, for the decoders that give a lane a bit stream of its
// own: the lane-per-member kernel (inflate_lane.hip) and the count-only size decode of the
// restart-point search (zs_sync.h).  The canonical code with its shape in registers or LDS, the
// direct root table, the code-length section of a dynamic block header and the fixed block's
// lengths.  Plain C++ on the lane reader but for the bit-reverse builtin and ZS_OPAQUE, so the host
// stand-ins of tools/lane_host, tools/lane_dict_host and tools/sync_host compile it too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_common.h"  // ZS_BL_ORDER
#include "zs_lane_reader.h"
#ifndef ZS_OPAQUE  // (the host stand-in of tools/lane_host defines it away)
#define ZS_OPAQUE(x) asm("" : "+v"(x))
#endif

// Canonical Huffman decoding (RFC 1951 3.2.2) with the code's shape in
// registers.  lim[l-1] is the end of the length-l codes left-justified to 15
// bits, so with the next 15 input bits read MSB first (rev), a code's length is
// one more than the number of limits <= rev, and its rank in (length, symbol)
// order is rev shifted down to that length plus D[length-1].  The symbols by
// rank are the only table, in LDS.  No memory access before the symbol itself
// and none in HBM: zlib's two-level tables (8-bit LDS roots before this) sent
// every code longer than the root to a second-level table in HBM, and some lane
// of a wave needed one in 68% of the C3 symbol steps -- a full memory latency
// for the whole wave each time.
struct zs_canon {
  uint32_t lim[15];
  uint32_t D[16];
};

// what zs_canon_build found.  zlib's inflate_table rejects over-subscribed sets and incomplete ones
// but for a lone code of length 1 outside the code-length code (inftrees.ts:128-139); a set without
// any code builds too, and no symbol decodes from it.  ZS_CODE_PARTIAL is those two: the unused
// codes answer "no such code" (every limit of a lone 1-bit code is 1 << 14, of an empty set 0).
enum { ZS_CODE_COMPLETE = 0, ZS_CODE_PARTIAL, ZS_CODE_REFUSED };

// C from lens[0..n) (LT: u16 in the lane kernel's HBM scratch, u8 in the sync lane's LDS), the
// symbols by rank in sym (ST u8: their low 8 bits, bit 8 in hi, one bit per rank; a wider ST holds
// them whole, hi = nullptr).  cnt: 16 words of LDS, left as the rank past the last code of each
// length.  codes: the code-length code.
template <class LT, class ST>
static __device__ int zs_canon_build(zs_canon& C, uint32_t* cnt, ST* sym, uint32_t* hi, const LT* lens, uint32_t n,
                                     bool codes) {
#pragma unroll
  for (int l = 0; l < 16; l++) cnt[l] = 0;
  if (hi)
#pragma unroll
    for (int w = 0; w < 9; w++) hi[w] = 0;
#pragma unroll 8
  for (uint32_t i = 0; i < n; i++) atomicAdd(&cnt[lens[i]], 1u);
  uint32_t code = 0, rank = 0;
  int left = 1;
#pragma unroll
  for (int l = 1; l <= 15; l++) {
    const uint32_t c = cnt[l];
    left = 2 * left - (int)c;  // once negative (over-subscribed) it stays so
    C.lim[l - 1] = (code + c) << (15 - l);
    C.D[l - 1] = rank - code;
    cnt[l] = rank;
    rank += c;
    code = (code + c) << 1;
  }
  C.D[15] = 0;
  int verdict = ZS_CODE_COMPLETE;
  if (left != 0) {  // (rank: the codes in all; lim[0]: those of length 1)
    if (left < 0 || !(rank == 0 || (!codes && rank == 1 && C.lim[0] == (1u << 14)))) return ZS_CODE_REFUSED;
    verdict = ZS_CODE_PARTIAL;
  }
#pragma unroll 8
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = lens[i];
    if (l) {
      const uint32_t k = atomicAdd(&cnt[l], 1u);
      sym[k] = (ST)i;
      if (hi && (i >> 8)) atomicOr(&hi[k >> 5], 1u << (k & 31u));
    }
  }
  return verdict;
}

// Direct root tables beside the canonical code: u16 entries length << 12 | symbol for every code
// of at most the root's bits, 0 = a longer code (or none), so most codes cost one LDS read.
#define ZS_LROOT 9u  // the literal/length root of both decoders, and the widest root zs_root_fill takes

// root[r] for every code of length <= rbits (after zs_canon_build: cnt[l] is
// the rank past the last length-l code, and a rank k of length l has code k - D[l-1])
template <class ST>
static __device__ void zs_root_fill(uint16_t* root, uint32_t rbits, const zs_canon& C, const uint32_t* cnt,
                                    const ST* sym, const uint32_t* hi) {
  for (uint32_t k = 0; k < (1u << rbits) / 2u; k++) reinterpret_cast<uint32_t*>(root)[k] = 0;
  uint32_t k = 0;
#pragma unroll
  for (uint32_t l = 1; l <= ZS_LROOT; l++) {
    if (l > rbits) break;
    const uint32_t end = cnt[l];
    for (; k < end; k++) {
      const uint32_t code = k - C.D[l - 1];
      const uint32_t r = __builtin_bitreverse32(code) >> (32u - l);  // the stream sends codes MSB first
      const uint32_t s = sym[k] | (hi ? ((hi[k >> 5] >> (k & 31u)) & 1u) << 8 : 0u);
      for (uint32_t x = r; x < (1u << rbits); x += 1u << l) root[x] = (uint16_t)((l << 12) | s);
    }
  }
}

// the rank of the code at the front of the bit buffer; L = its length (16: no
// such code -- the caller bails)
static __device__ __forceinline__ uint32_t zs_canon_rank(const zs_canon& C, const zs_lane_reader& R, uint32_t& L) {
  const uint32_t rev = __builtin_bitreverse32((uint32_t)R.hold) >> 17;
  // the values pass an empty asm so each select below is between registers (the
  // compiler otherwise selects an address into C and keeps C in scratch)
  uint32_t d[16];
#pragma unroll
  for (int l = 0; l < 16; l++) {
    d[l] = C.D[l];
    ZS_OPAQUE(d[l]);
  }
  uint32_t n = 1, D = d[0];
#pragma unroll
  for (int l = 0; l < 15; l++) {
    const bool c = rev >= C.lim[l];
    n += c;
    D = c ? d[l + 1] : D;
  }
  L = n;
  return (rev >> ((15u - n) & 31u)) + D;
}
// the same from a code kept in LDS: the limits in four 16-byte reads, then the
// one D[] entry of the code's length
static __device__ __forceinline__ uint32_t zs_canon_rank_lds(const zs_canon& C, const zs_lane_reader& R,
                                                             uint32_t& L) {
  const uint32_t rev = __builtin_bitreverse32((uint32_t)R.hold) >> 17;
  const uint4* l4 = reinterpret_cast<const uint4*>(C.lim);  // lim[0..14] (+ D[0], unused)
  const uint4 q0 = l4[0], q1 = l4[1], q2 = l4[2], q3 = l4[3];
  const uint32_t lim[15] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z};
  uint32_t n = 1;
#pragma unroll
  for (int l = 0; l < 15; l++) n += rev >= lim[l] ? 1u : 0u;
  L = n;
  return (rev >> ((15u - n) & 31u)) + C.D[(n - 1u) & 15u];
}
template <bool LDS>
static __device__ __forceinline__ uint32_t zs_canon_rank_t(const zs_canon& C, const zs_lane_reader& R, uint32_t& L) {
  if constexpr (LDS) return zs_canon_rank_lds(C, R, L);
  else return zs_canon_rank(C, R, L);
}

// a fixed block's lengths (inflate.ts:218-280): 288 literal/length codes, then 32 distance codes
template <class LT>
static __device__ __forceinline__ void zs_lane_fixed_lengths(LT* lens) {
  for (uint32_t sym = 0; sym < 320; sym++) lens[sym] = (LT)(sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : sym < 288 ? 8 : 5);
}

// The code-length section of a dynamic block header (inflate.ts:662-836), the reader behind the
// block's type bits: HLIT / HDIST / HCLEN, the code-length code (built into C, cnt and sym8, which
// the caller reuses for the block's own codes; LDS: C lies in LDS), then lens[0..nlen + ndist).
// d64: deflate64, whose distance code has up to 32 symbols.  false: zlib refuses the header -- too
// many symbols, a code-length code that is over-subscribed or incomplete, a code that does not
// exist, a repeat with nothing before it or past the end, no end-of-block code.  That last test is
// made only of a header that lies inside the input: whether the reader has run past it is the
// caller's test, which follows the call.
template <bool LDS, class LT>
static __device__ __forceinline__ bool zs_lane_code_lengths(zs_lane_reader& R, bool d64, zs_canon& C, uint32_t* cnt,
                                                            uint8_t* sym8, LT* lens, uint32_t& nlen, uint32_t& ndist) {
  nlen = zs_lr_take(R, 5) + 257;
  ndist = zs_lr_take(R, 5) + 1;
  const uint32_t ncode = zs_lr_take(R, 4) + 4;
  if (nlen > 286 || (!d64 && ndist > 30)) return false;
  uint32_t i;
  for (i = 0; i < ncode; i++) lens[ZS_BL_ORDER[i]] = (LT)zs_lr_take(R, 3);
  for (; i < 19; i++) lens[ZS_BL_ORDER[i]] = 0;
  // (an empty code-length code builds; its first symbol then does not exist)
  if (zs_canon_build(C, cnt, sym8, nullptr, lens, 19, true) == ZS_CODE_REFUSED) return false;
  i = 0;
  uint32_t prev = 0;
  while (i < nlen + ndist) {
    if (R.bits < 32) zs_lr_fill(R);
    uint32_t L;
    const uint32_t k = zs_canon_rank_t<LDS>(C, R, L);
    if (L > 15) return false;
    zs_lr_drop(R, L);
    const uint32_t v = sym8[k];
    if (v < 16) {
      lens[i++] = (LT)v;
      prev = v;
      continue;
    }
    uint32_t rep, val = 0;
    if (v == 16) {
      if (i == 0) return false;
      val = prev;
      rep = 3 + zs_lr_take(R, 2);
    } else if (v == 17) {
      rep = 3 + zs_lr_take(R, 3);
    } else {
      rep = 11 + zs_lr_take(R, 7);
    }
    if (i + rep > nlen + ndist) return false;
    while (rep--) lens[i++] = (LT)val;
    prev = val;
  }
  return zs_lr_over(R) || lens[256] != 0;  // "missing end-of-block"
}
