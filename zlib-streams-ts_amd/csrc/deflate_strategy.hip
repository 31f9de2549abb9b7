// deflate_strategy.hip -- the tallies of the strategies that search no hash chains:
// Z_HUFFMAN_ONLY (deflate_huff, deflate.ts:1525-1565) and Z_RLE (deflate_rle,
// deflate.ts:1450-1523 as zlib runs it: option rle_ref = 0).  They write what the parse
// kernels write -- the stream's symbols, its block records (a block closes after every
// 16,383rd symbol, deflate.ts:336; the last one is final, possibly empty) and
// zs_stream.nsym / nblk -- and zs_k_trees onwards runs unchanged.
#include <hip/hip_runtime.h>
#include "zs_common.h"
#include "zs_kernels.h"
#include "zs_rle.h"

static __device__ __forceinline__ zs_block zs_tally_block(uint32_t b, uint32_t sym_count, uint32_t in_start,
                                                          uint32_t in_end, uint32_t last) {
  zs_block k;
  k.sym_start = b * ZS_SYM_END;
  k.sym_count = sym_count;
  k.in_start = in_start;
  k.in_end = in_end;
  k.type = 0; k.hdr_bits = 0; k.data_bits = 0; k.pad = 0; k.bit_off = 0; k.bit_end = 0;
  k.last = last;
  return k;
}

// ------------------------------------------------------------- Z_HUFFMAN_ONLY
// Every byte is a literal: block b of a stream covers the input [16383 b, min(n,
// 16383 (b + 1))) and as many symbols.  One workgroup per (stream, block) pair of the
// host's list: a widening copy of the block's bytes to u32 symbols -- each lane reads
// 4 bytes (a wave 256 contiguous bytes) and stores one 16-byte quad (a wave 1 KiB);
// quads are aligned to the symbol array's 16 bytes, the ragged ones at the block's two
// ends go byte by byte.  A block never starts before the slid window (its input is
// at most 16,383 bytes back when fill_window slides), so bit 1 of `last` stays clear.
#define ZS_HUFF_THREADS 256u
#define ZS_HUFF_UNROLL 4u
__global__ __launch_bounds__(ZS_HUFF_THREADS) void zs_k_huff_tally(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len,
    const uint64_t* __restrict__ pos_base, const uint32_t* __restrict__ blk_base,
    const zs_huff_chunk* __restrict__ chunks, uint32_t* __restrict__ syms, zs_block* __restrict__ blocks,
    zs_stream* __restrict__ streams) {
  const zs_huff_chunk c = chunks[blockIdx.x];
  const uint32_t s = c.s, b = c.b, n = in_len[s];
  const uint32_t lo = b * ZS_SYM_END, hi = min(n, lo + ZS_SYM_END);  // lo <= n: the host lists n / 16383 + 1 blocks
  const uint32_t nblk = n / ZS_SYM_END + 1;
  if (threadIdx.x == 0) {
    blocks[blk_base[s] + b] = zs_tally_block(b, hi - lo, lo, hi, b + 1 == nblk ? 1u : 0u);
    if (b == 0) {
      streams[s].nsym = n;
      streams[s].nblk = nblk;
    }
  }
  const uint8_t* src = in + in_off[s];
  const uint64_t g0 = pos_base[s] + s;  // the stream's first symbol slot (u32 index)
  // quads of the symbol array (u32 index 4 q .. 4 q + 3) that hold a symbol of [lo, hi)
  const uint64_t q_lo = (g0 + lo) >> 2, q_hi = (g0 + hi + 3) >> 2;
  const bool aligned = (((uintptr_t)src - g0) & 3u) == 0;  // a quad's four bytes (src + 4 q - g0) are an aligned word
  for (uint64_t q0 = q_lo; q0 < q_hi; q0 += ZS_HUFF_THREADS * ZS_HUFF_UNROLL) {
    uint32_t w[ZS_HUFF_UNROLL];
    // every load before the first store (stores share the loads' counter on gfx9)
#pragma unroll
    for (uint32_t k = 0; k < ZS_HUFF_UNROLL; k++) {
      const uint64_t q = q0 + k * ZS_HUFF_THREADS + threadIdx.x;
      w[k] = 0;
      if (q >= q_hi) continue;
      const int64_t i0 = (int64_t)(4 * q) - (int64_t)g0;  // the quad's first symbol = input position
      if (i0 >= (int64_t)lo && i0 + 4 <= (int64_t)hi) {
        if (aligned) w[k] = *reinterpret_cast<const uint32_t*>(src + i0);
        else w[k] = (uint32_t)src[i0] | (uint32_t)src[i0 + 1] << 8 | (uint32_t)src[i0 + 2] << 16 | (uint32_t)src[i0 + 3] << 24;
      } else {
        for (int j = 0; j < 4; j++)
          if (i0 + j >= (int64_t)lo && i0 + j < (int64_t)hi) w[k] |= (uint32_t)src[i0 + j] << (8 * j);
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < ZS_HUFF_UNROLL; k++) {
      const uint64_t q = q0 + k * ZS_HUFF_THREADS + threadIdx.x;
      if (q >= q_hi) continue;
      const int64_t i0 = (int64_t)(4 * q) - (int64_t)g0;
      if (i0 >= (int64_t)lo && i0 + 4 <= (int64_t)hi) {
        *reinterpret_cast<uint4*>(syms + 4 * q) =
            make_uint4(w[k] & 0xffu, (w[k] >> 8) & 0xffu, (w[k] >> 16) & 0xffu, w[k] >> 24);
      } else {
        for (int j = 0; j < 4; j++)
          if (i0 + j >= (int64_t)lo && i0 + j < (int64_t)hi) syms[4 * q + j] = (w[k] >> (8 * j)) & 0xffu;
      }
    }
  }
}

// ---------------------------------------------------------------------- Z_RLE
// zlib's deflate_rle (option rle_ref = 0): greedy matches at distance 1, in the closed
// form of zs_rle.h -- the symbol that starts at a position follows from the position,
// its run's start and the run's end within the next 258 bytes, so no lane walks a
// stream.  One workgroup per stream, over tiles of ZS_RLE_TILE positions:
//   1. the tile's bytes, the byte before and ZS_RLE_HALO bytes behind (aligned words) to LDS;
//   2. run starts, in[p] != in[p - 1] (and p = 0, and every p >= n), by wave ballots into a
//      bit map of tile + halo; the last start at or before each 64-position word by a
//      wave scan, seeded with the CARRY: the start of the run that enters the tile;
//   3. per position: run start (the word's bits below, else the scan), run end (the next
//      set bit, searched at most 258 positions ahead), zs_rle_at; the symbols' ballot;
//   4. the symbols' offsets by a scan of the ballots' popcounts; a compacting store; the
//      symbol that is a block's 16,383rd records the block's input end.
// Then the block records, as the parse kernels write them.  Bit 1 of `last` (the block
// began before the slid window: a stored block of it is not reproducible) is set from
// an upper bound of the slides by the block's end -- fill_window slides no earlier than
// position 65,274 + 32,768 j -- which no block of literals alone (16,383 bytes) reaches.
#define ZS_RLE_THREADS 256u
#define ZS_RLE_TILE 4096u
#define ZS_RLE_HALO 320u  // >= 258, whole 64-position words
#define ZS_RLE_WORDS ((ZS_RLE_TILE + ZS_RLE_HALO) / 64u)  // 69
#define ZS_RLE_PER (ZS_RLE_TILE / ZS_RLE_THREADS)        // positions per thread (16)
static_assert(ZS_RLE_HALO >= ZS_RLE_MAX && ZS_RLE_HALO % 64u == 0 && ZS_RLE_WORDS <= 128u, "halo");

struct zs_rle_lds {
  uint32_t bytes[(ZS_RLE_TILE + ZS_RLE_HALO + 8u) / 4u + 1u];  // byte k: position t0 - 1 - A + k (A: the word misalignment)
  uint64_t start[ZS_RLE_WORDS];   // run-start bits of tile + halo
  uint32_t before[ZS_RLE_WORDS];  // last start in the words before word w (or the carry)
  uint64_t emit[ZS_RLE_TILE / 64u];
  uint32_t off[ZS_RLE_TILE / 64u + 1u];  // exclusive prefix of the emit popcounts
};

__global__ __launch_bounds__(ZS_RLE_THREADS) void zs_k_rle_tally(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len,
    const uint64_t* __restrict__ pos_base, const uint32_t* __restrict__ blk_base, uint32_t* __restrict__ syms,
    zs_block* __restrict__ blocks, zs_stream* __restrict__ streams) {
  __shared__ zs_rle_lds S;
  const uint32_t s = blockIdx.x;
  const uint32_t n = in_len[s];
  const uint8_t* src = in + in_off[s];
  uint32_t* sy = syms + pos_base[s] + s;
  zs_block* blk = blocks + blk_base[s];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint8_t* lb = reinterpret_cast<const uint8_t*>(S.bytes);
  uint32_t total = 0;  // symbols written (uniform)
  uint32_t carry = 0;  // start of the run of position t0 - 1 (uniform)

  for (uint32_t t0 = 0; t0 < n; t0 += ZS_RLE_TILE) {
    // ---- 1. bytes [t0 - 1, t0 + TILE + HALO) in aligned words; a word is loaded when it holds a byte of the stream
    const uintptr_t first = (uintptr_t)src + t0 - 1;  // (t0 = 0: the byte before the stream is never used)
    const uint32_t A = (uint32_t)(first & 3u);
    const uint8_t* wbase = reinterpret_cast<const uint8_t*>(first - A);
    for (uint32_t k = threadIdx.x; k < (ZS_RLE_TILE + ZS_RLE_HALO + 8u) / 4u; k += ZS_RLE_THREADS) {
      const uint8_t* wp = wbase + 4 * k;
      S.bytes[k] = (wp + 4 > src && wp < src + n) ? *reinterpret_cast<const uint32_t*>(wp) : 0u;
    }
    __syncthreads();
    auto byte_at = [&](uint32_t p) { return (uint32_t)lb[p - t0 + 1u + A]; };  // t0 - 1 <= p < t0 + TILE + HALO
    // ---- 2. run starts
    for (uint32_t w = wave; w < ZS_RLE_WORDS; w += ZS_RLE_THREADS / 64u) {
      const uint32_t p = t0 + 64u * w + lane;
      const bool st = p >= n || p == 0 || byte_at(p) != byte_at(p - 1);
      const uint64_t m = __builtin_amdgcn_ballot_w64(st);
      if (lane == 0) S.start[w] = m;
    }
    __syncthreads();
    if (wave == 0) {
      uint32_t prev = carry;  // the last start before the words of this round
      for (uint32_t w0 = 0; w0 < ZS_RLE_WORDS; w0 += 64) {
        const uint32_t w = w0 + lane;
        const uint64_t m = w < ZS_RLE_WORDS ? S.start[w] : 0ull;
        uint32_t v = m ? t0 + 64u * w + 63u - (uint32_t)__builtin_clzll(m) : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t y = __shfl_up(v, d, 64);
          if (lane >= (uint32_t)d) v = max(v, y);
        }
        v = max(v, prev);
        const uint32_t up = __shfl_up(v, 1, 64);
        if (w < ZS_RLE_WORDS) S.before[w] = lane == 0 ? prev : up;
        prev = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
      }
    }
    __syncthreads();
    // ---- 3. the symbol that starts at each position of the tile
    uint32_t v[ZS_RLE_PER];
#pragma unroll
    for (uint32_t k = 0; k < ZS_RLE_PER; k++) {
      const uint32_t w = wave + k * (ZS_RLE_THREADS / 64u);
      const uint32_t p = t0 + 64u * w + lane;
      uint32_t sym = ZS_RLE_NONE;
      if (p < n) {
        const uint64_t m = S.start[w];
        const uint64_t le = m & (~0ull >> (63u - lane));
        const uint32_t rs = le ? t0 + 64u * w + 63u - (uint32_t)__builtin_clzll(le) : S.before[w];
        // the run's end: the next start (every position from n on is one), looked for up to 258 ahead
        uint64_t gt = lane == 63u ? 0ull : m & (~0ull << (lane + 1u));
        uint32_t we = w;
        while (!gt && we + 1 < ZS_RLE_WORDS && 64u * (we + 1) <= 64u * w + lane + ZS_RLE_MAX) gt = S.start[++we];
        const uint64_t e = gt ? (uint64_t)t0 + 64u * we + (uint32_t)__builtin_ctzll(gt) : (uint64_t)p + 2u * ZS_RLE_MAX;
        sym = zs_rle_at(p, rs, e, byte_at(p));
      }
      v[k] = sym;
      const uint64_t em = __builtin_amdgcn_ballot_w64(sym != ZS_RLE_NONE);
      if (lane == 0) S.emit[w] = em;
    }
    __syncthreads();
    // ---- 4. offsets, the compacting store, block cuts
    if (wave == 0) {
      uint32_t c = (uint32_t)__builtin_popcountll(S.emit[lane]), incl = c;  // TILE / 64 = 64 words
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += y;
      }
      S.off[lane] = incl - c;
      if (lane == 63) S.off[64] = incl;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ZS_RLE_PER; k++) {
      if (v[k] == ZS_RLE_NONE) continue;
      const uint32_t w = wave + k * (ZS_RLE_THREADS / 64u);
      const uint32_t p = t0 + 64u * w + lane;
      const uint32_t g = total + S.off[w] + (uint32_t)__builtin_popcountll(S.emit[w] & ((1ull << lane) - 1ull));
      sy[g] = v[k];  // g < n: a symbol per position at most
      if ((g + 1) % ZS_SYM_END == 0)  // FLUSH_BLOCK after this symbol: block_start = strstart behind it
        blk[(g + 1) / ZS_SYM_END - 1].in_end = p + ((v[k] & 0x80000000u) ? ((v[k] >> 16) & 0xffu) + ZS_MIN_MATCH : 1u);
    }
    total += S.off[ZS_RLE_TILE / 64u];
    carry = max(carry, max(S.before[ZS_RLE_TILE / 64u - 1u],
                           S.start[ZS_RLE_TILE / 64u - 1u]
                               ? t0 + ZS_RLE_TILE - 1u - (uint32_t)__builtin_clzll(S.start[ZS_RLE_TILE / 64u - 1u])
                               : 0u));
    __syncthreads();  // the tile's LDS is read to here
  }

  // ---- block records (the final block takes the rest, possibly empty)
  __threadfence_block();
  __syncthreads();
  const uint32_t nflush = total / ZS_SYM_END;
  for (uint32_t b0 = 0; b0 <= nflush; b0 += ZS_RLE_THREADS) {
    const uint32_t b = b0 + threadIdx.x;
    zs_block k;
    if (b <= nflush) {
      const uint32_t in_start = b == 0 ? 0u : blk[b - 1].in_end;
      const uint32_t in_end = b < nflush ? blk[b].in_end : n;
      const uint32_t slides = in_end >= ZS_SLIDE_AT ? (in_end - ZS_SLIDE_AT) / 32768u + 1u : 0u;  // an upper bound
      k = zs_tally_block(b, b < nflush ? ZS_SYM_END : total - nflush * ZS_SYM_END, in_start, in_end,
                         (b == nflush ? 1u : 0u) | ((uint64_t)in_start < 32768ull * slides ? 2u : 0u));
    }
    __syncthreads();  // every read of in_end in this chunk precedes the writes
    if (b <= nflush) blk[b] = k;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    streams[s].nsym = total;
    streams[s].nblk = nflush + 1;
  }
}
