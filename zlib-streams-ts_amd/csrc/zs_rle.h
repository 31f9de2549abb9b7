// zs_rle.h -- the closed form of zlib's deflate_rle parse (deflate.c 1.2.11; the
// reference's deflate_rle, deflate.ts:1450-1523, but for its scan comparing the
// previous byte's VALUE with the scan INDEX, deflate.ts:1469-1481, which never
// finds a run -- SURVEY.md; option rle_ref).  Plain arithmetic, no HIP types: the
// tally kernel (deflate_strategy.hip) and the host check (tools/emu/emu_rle.cpp,
// tests/test_rle_model.py) compile the same functions.
//
// deflate_rle is greedy with distance 1: at position p > 0 with in[p-1] == in[p]
// == in[p+1] == in[p+2] it tallies a match of the bytes equal to in[p-1] from p
// on, at most 258 (lookahead is above 258 whenever input remains, so it never
// shortens a match); else the literal in[p].  Per MAXIMAL RUN of one byte value,
// starting at s with length L, that is:
//   - position s is a literal (it differs from in[s-1]; s = 0 fails strstart > 0);
//   - the m = L - 1 bytes behind it go in groups of 258 from s + 1: a group with
//     g >= 3 bytes left in the run is one match (min(g, 258), distance 1), a last
//     group of 1 or 2 bytes is that many literals.
// The end of the stream needs no case of its own: a run cannot pass it.
#ifndef ZS_RLE_H
#define ZS_RLE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define ZS_RLE_FN static __host__ __device__ inline
#else
#define ZS_RLE_FN static inline
#endif

#define ZS_RLE_MAX 258u         // MAX_MATCH
#define ZS_RLE_MIN 3u           // MIN_MATCH
#define ZS_RLE_NONE 0xffffffffu  // no symbol starts here

// a match of len bytes at distance 1, as the parse kernels write it
ZS_RLE_FN uint32_t zs_rle_match(uint32_t len) { return 0x80000000u | ((len - ZS_RLE_MIN) << 16) | 1u; }

// symbols of a run of L >= 1 bytes
ZS_RLE_FN uint32_t zs_rle_run_syms(uint64_t L) {
  const uint64_t m = L - 1, q = m / ZS_RLE_MAX, r = m % ZS_RLE_MAX;
  return (uint32_t)(1 + q + (r >= ZS_RLE_MIN ? 1 : r));
}

// the k-th symbol (k < zs_rle_run_syms(L)) of the run at s: its offset from s; *len its
// bytes (1: a literal)
ZS_RLE_FN uint64_t zs_rle_run_sym_at(uint64_t L, uint32_t k, uint32_t* len) {
  const uint64_t m = L - 1, q = m / ZS_RLE_MAX, r = m % ZS_RLE_MAX;
  *len = 1;
  if (k == 0) return 0;
  if (k <= q) {
    *len = ZS_RLE_MAX;
    return 1 + (uint64_t)(k - 1) * ZS_RLE_MAX;
  }
  if (r >= ZS_RLE_MIN) {
    *len = (uint32_t)r;
    return 1 + q * ZS_RLE_MAX;
  }
  return 1 + q * ZS_RLE_MAX + (k - q - 1);
}

// The symbol that STARTS at position p (ZS_RLE_NONE: p is inside a match), given
// p's byte, the start s <= p of its run and the run's end e > p (exclusive).  Only
// min(e, p + 258) matters, so a caller that looks 258 bytes past p may pass any
// larger value for a run that ends beyond.
ZS_RLE_FN uint32_t zs_rle_at(uint32_t p, uint32_t s, uint64_t e, uint32_t byte) {
  if (p == s) return byte;
  const uint32_t g0 = s + 1 + (p - s - 1) / ZS_RLE_MAX * ZS_RLE_MAX;  // p's group of 258
  const uint64_t left = e - g0;
  if (left < ZS_RLE_MIN) return byte;
  if (p != g0) return ZS_RLE_NONE;
  return zs_rle_match(left < ZS_RLE_MAX ? (uint32_t)left : ZS_RLE_MAX);
}

#endif
