// zs_wave.h -- what the wave-uniform decoders share: the wave-per-member inflate
// kernel (inflate_wave.hip), the split decode of large members
// (inflate_split.hip) and the segmented walk (inflate_seg.hip).  The bit reader
// with every value in SGPRs, its set-up (zs_wr_init, zs_wr_start), the plain
// zlib / gzip wrapper header (zs_wr_wrapper_header) and the one deflate block
// header parse on that reader (zs_wr_block_header).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_common.h"
#include "zs_inftab.h"
#include "zs_refcalls.h"

#ifndef ZS_WIN_IN
#define ZS_WIN_IN 256u  // staged input words
#endif

static __device__ __forceinline__ uint32_t zs_u(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// wave-uniform bit reader: the zs_lane_reader scheme (clamped aligned words,
// one refill ahead) with every value in SGPRs.  The input words are staged in
// LDS, 1 KiB at a time by the whole wave: a refill is then an LDS read, which
// the table lookups' waits cover, where a direct load would wait behind the
// output stores (vmcnt) or -- as a scalar load -- make every table lookup's
// lgkmcnt wait for it.
struct zs_wave_reader {
  const uint32_t* w4;  // the aligned words holding the member's bytes
  uint32_t* inw;       // LDS: words [qb, qb + ZS_WIN_IN) of w4 (clamped to `last`)
  uint32_t qb;
  uint32_t sh, last, n, pos;
  uint64_t hold;
  uint32_t bits;
  uint32_t pf;
};

// the member: n > 0 bytes at src, staged through inw (an empty member's reader
// must not read its own address: the caller points w4 at a word it may read,
// with last = 0)
static __device__ __forceinline__ void zs_wr_init(zs_wave_reader& R, const uint8_t* src, uint32_t n, uint32_t* inw) {
  R.n = n;
  R.sh = (uint32_t)((uintptr_t)src & 3u);
  R.w4 = reinterpret_cast<const uint32_t*>(src - R.sh);
  R.last = (R.sh + n - 1u) >> 2;
  R.inw = inw;
}
static __device__ __forceinline__ void zs_wr_stage(zs_wave_reader& R, uint32_t q) {
  R.qb = q;
#pragma unroll 4
  for (uint32_t i = threadIdx.x; i < ZS_WIN_IN; i += 64) R.inw[i] = R.w4[min(q + i, R.last)];
}
static __device__ __forceinline__ uint32_t zs_wr_load4(zs_wave_reader& R, uint32_t at) {
  const uint32_t q = (at + R.sh) >> 2;
  if (q + 1u >= R.qb + ZS_WIN_IN) zs_wr_stage(R, q);
  const uint32_t lo = zs_u(R.inw[q - R.qb]), hi = zs_u(R.inw[q + 1u - R.qb]);
  // (at + sh) & 3 is sh except after a stored block's seek
  const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * ((at + R.sh) & 3u)));
  const uint32_t valid = at < R.n ? R.n - at : 0u;
  return valid >= 4u ? v : v & ((1u << (8u * valid)) - 1u);
}
static __device__ __forceinline__ void zs_wr_fill(zs_wave_reader& R) {
  R.hold |= (uint64_t)R.pf << R.bits;
  R.bits += 32;
  R.pos += 4;
  R.pf = zs_wr_load4(R, R.pos);
}
static __device__ __forceinline__ uint64_t zs_wr_bitpos(const zs_wave_reader& R) { return (uint64_t)R.pos * 8u - R.bits; }
static __device__ __forceinline__ bool zs_wr_over(const zs_wave_reader& R) { return zs_wr_bitpos(R) > (uint64_t)R.n * 8u; }
static __device__ __forceinline__ uint32_t zs_wr_take(zs_wave_reader& R, uint32_t k) {  // k <= 32
  if (R.bits < k) zs_wr_fill(R);
  const uint32_t v = (uint32_t)R.hold & (k == 32 ? 0xffffffffu : ((1u << k) - 1));
  R.hold >>= k;
  R.bits -= k;
  return v;
}
static __device__ __forceinline__ void zs_wr_align(zs_wave_reader& R) {
  const uint32_t d = R.bits & 7u;
  R.hold >>= d;
  R.bits -= d;
}
// restart the reader at byte `at` (after a stored block copied straight from the input)
static __device__ __forceinline__ void zs_wr_seek(zs_wave_reader& R, uint32_t at) {
  R.pos = at;
  R.hold = 0;
  R.bits = 0;
  R.pf = zs_wr_load4(R, at);
}
static __device__ __forceinline__ zcode zs_wr_decode(zs_wave_reader& R, const zcode* t, uint32_t rbits) {
  if (R.bits < 32) zs_wr_fill(R);
  zcode here = zs_u(t[(uint32_t)R.hold & ((1u << rbits) - 1)]);
  if (C_OP(here) && (C_OP(here) & 0xf0) == 0) {  // second-level table
    const uint32_t rb = C_BITS(here);
    const zcode last = here;
    here = zs_u(t[C_VAL(last) + (((uint32_t)R.hold & ((1u << (rb + C_OP(last))) - 1)) >> rb)]);
    R.hold >>= rb;
    R.bits -= rb;
  }
  R.hold >>= C_BITS(here);
  R.bits -= C_BITS(here);
  return here;
}
// start reading at any bit of the member (its staging window from there)
static __device__ __forceinline__ void zs_wr_start(zs_wave_reader& R, uint64_t bit) {
  const uint32_t at = (uint32_t)(bit >> 3);
  zs_wr_stage(R, (at + R.sh) >> 2);
  zs_wr_seek(R, at);
  zs_wr_take(R, (uint32_t)bit & 7u);
}

// The wrapper header (inflate.ts:377-580) of a zlib / gzip member (wrap != 0,
// inflate.ts:152-160): plain headers only -- gzip header fields, FDICT or a
// failed check are false, and the exact path reports them.  extra_ok (zlib
// semantics: no call of the reference's to reproduce): a gzip header whose one
// flag is FEXTRA -- a BGZF block, DESIGN 4.15 -- is taken too, the field skipped
// whatever it holds, as the lane path does; a field that passes the input leaves
// the reader past its end, which the block header behind it refuses.
static __device__ __forceinline__ bool zs_wr_wrapper_header(zs_wave_reader& R, int wrap, bool extra_ok) {
  const uint32_t b0 = zs_wr_take(R, 8), b1 = zs_wr_take(R, 8);
  if ((wrap & 2) && b0 == 0x1f && b1 == 0x8b) {
    const uint32_t cm = zs_wr_take(R, 8), flg = zs_wr_take(R, 8);
    zs_wr_take(R, 32);  // MTIME
    zs_wr_take(R, 16);  // XFL, OS
    if (cm == 8 && flg == 4 && extra_ok) {
      const uint32_t xlen = zs_wr_take(R, 16);
      zs_wr_start(R, 8ull * (12u + xlen));
      return true;
    }
    return cm == 8 && flg == 0;
  }
  if (wrap & 1) return !(((b0 << 8) | b1) % 31 || (b0 & 15) != 8 || (b0 >> 4) + 8 > 15 || (b1 & 0x20));
  return false;  // "incorrect header check"
}

// a wave-uniform decoder's LDS besides its history ring: the staged input and zlib's tables
struct zs_wave_tabs {
  uint32_t inw[ZS_WIN_IN];
  zcode codes[ENOUGH_LENS + ENOUGH_DISTS_9];
  uint16_t lens[320];
  uint16_t work[288];
};

// The block header at the reader's position (inflate.ts:600-836) into zlib's
// tables (inflate_table) in LDS: the literal/length table at codes (root
// lbits), the distance table at codes + dofs (root dbits), ntab entries in all.
// A stored block's length (inflate.ts:631-672: LEN and NLEN at the next byte
// boundary, the reader left at its first byte) comes back in slen, else
// ZS_WR_CODED.  false for anything invalid.  All 64 lanes run it on identical
// values.  WAVE_TABLES: the tables from zs_inflate_table_wave (the segmented
// walk: any code set but a complete one is invalid there), else from the
// serial inflate_table (the wave and split decoders: incomplete codes as zlib
// accepts them, and their occupancy, see zs_inftab.h).
#define ZS_WR_CODED 0xffffffffu
template <bool WAVE_TABLES>
static __device__ __forceinline__ int zs_wr_table(int type, const uint16_t* lens, uint32_t n, zcode* table,
                                                  uint32_t* bits, uint16_t* work, bool d64, uint32_t* used) {
  if constexpr (WAVE_TABLES) return zs_inflate_table_wave<false>(type, lens, n, table, bits, work, d64, used);
  else return zs_inflate_table(type, lens, n, table, bits, work, d64, used);
}
template <bool WAVE_TABLES>
static __device__ bool zs_wr_block_header(zs_wave_reader& R, zcode* codes, uint16_t* lens, uint16_t* work, bool d64,
                                          uint32_t& last, uint32_t& lbits, uint32_t& dbits, uint32_t& dofs,
                                          uint32_t& ntab, uint32_t& slen) {
  last = zs_wr_take(R, 1);
  const uint32_t type = zs_wr_take(R, 2);
  uint32_t lused = 0, dused = 0;
  slen = ZS_WR_CODED;
  if (type == 0) {
    zs_wr_align(R);
    const uint32_t len = zs_wr_take(R, 16), nlen = zs_wr_take(R, 16);
    if (len != (nlen ^ 0xffffu) || zs_wr_over(R)) return false;  // "invalid stored block lengths", or past the input
    slen = len;
    return true;
  }
  if (type == 1) {  // fixed tables (inflate.ts:218-280)
    uint32_t sym;
    for (sym = 0; sym < 144; sym++) lens[sym] = 8;
    for (; sym < 256; sym++) lens[sym] = 9;
    for (; sym < 280; sym++) lens[sym] = 7;
    for (; sym < 288; sym++) lens[sym] = 8;
    lbits = 9;
    zs_wr_table<WAVE_TABLES>(LENS, lens, 288, codes, &lbits, work, d64, &lused);
    for (sym = 0; sym < 32; sym++) lens[sym] = 5;
    dbits = 5;
    zs_wr_table<WAVE_TABLES>(DISTS, lens, 32, codes + lused, &dbits, work, d64, &dused);
  } else if (type == 2) {  // dynamic (inflate.ts:662-836)
    const uint32_t nlen = zs_wr_take(R, 5) + 257, ndist = zs_wr_take(R, 5) + 1, ncode = zs_wr_take(R, 4) + 4;
    if (nlen > 286 || (!d64 && ndist > 30)) return false;
    uint32_t i;
    for (i = 0; i < ncode; i++) lens[ZS_BL_ORDER[i]] = (uint16_t)zs_wr_take(R, 3);
    for (; i < 19; i++) lens[ZS_BL_ORDER[i]] = 0;
    uint32_t cbits = 7, used;
    if (zs_wr_table<WAVE_TABLES>(CODES, lens, 19, codes, &cbits, work, d64, &used)) return false;
    // The code lengths (inflate.ts:702-778), one symbol at a time but with no
    // memory round trip per symbol: the code-length code's table (<= 128
    // entries of bits << 8 | symbol) sits in a VGPR, lane l holding entries l
    // and l + 64, read with v_readlane at the input's next cbits bits; a repeat
    // is stored by up to 138 lanes at once; the previous length stays in a
    // register.  (Was an LDS lookup and readfirstlane per symbol and a store
    // per repeated length: ~44k core cycles per header, profiles/r06/hdr/.)
    const uint32_t lane = threadIdx.x & 63u, csz = 1u << cbits, cmask = csz - 1u, N = nlen + ndist;
    const zcode c0 = lane < csz ? codes[lane] : 0u, c1 = lane + 64u < csz ? codes[lane + 64u] : 0u;
    const uint32_t tv = ((C_BITS(c0) << 8) | C_VAL(c0)) | (((C_BITS(c1) << 8) | C_VAL(c1)) << 16);
    uint32_t prev = 0;
    i = 0;
    while (i < N) {
      if (R.bits < 32) zs_wr_fill(R);
      const uint32_t idx = (uint32_t)R.hold & cmask;
      const uint32_t e2 = (uint32_t)__builtin_amdgcn_readlane((int)tv, (int)(idx & 63u));
      const uint32_t e = (idx & 64u) ? e2 >> 16 : e2 & 0xffffu;
      const uint32_t nb = e >> 8, v = e & 0xffu;
      R.hold >>= nb;
      R.bits -= nb;
      if (v < 16) {
        lens[i++] = (uint16_t)v;
        prev = v;
        continue;
      }
      uint32_t rep, val = 0;
      if (v == 16) {
        if (i == 0) return false;
        val = prev;
        rep = 3 + zs_wr_take(R, 2);
      } else if (v == 17) {
        rep = 3 + zs_wr_take(R, 3);
      } else {
        rep = 11 + zs_wr_take(R, 7);
      }
      if (i + rep > N) return false;
      for (uint32_t j = lane; j < rep; j += 64u) lens[i + j] = (uint16_t)val;
      i += rep;
      prev = val;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // (the lengths visible to this wave's table builds)
    __builtin_amdgcn_wave_barrier();
    if (zs_wr_over(R) || zs_u(lens[256]) == 0) return false;
    lbits = 9;
    if (zs_wr_table<WAVE_TABLES>(LENS, lens, nlen, codes, &lbits, work, d64, &lused)) return false;
    dbits = 6;
    if (zs_wr_table<WAVE_TABLES>(DISTS, lens + nlen, ndist, codes + lused, &dbits, work, d64, &dused)) return false;
  } else {
    return false;  // "invalid block type"
  }
  lbits = zs_u(lbits);
  dbits = zs_u(dbits);
  dofs = zs_u(lused);
  ntab = zs_u(lused + dused);
  return true;
}
