// zs_sweep_ring.h -- the slot, mirror, validity and run arithmetic of
// zs_k_sweep's persistent per-wave ring (deflate_sweep.hip, chain <= 128:
// levels 4..6).  Plain inline functions for the kernel and for the host model
// that replays the ring's writes and reads (tools/emu/emu_sweep_ring.c,
// tests/test_sweep_ring_model.py).
//
// A wave claims a RUN of consecutive 64-member chunks.  Chunk c's lanes hold
// members 64c .. 64c + 63 (block c) and read, for chain step t, member k - t:
// with chain <= 128 that is blocks c, c - 1 and c - 2.  The ring holds three
// blocks: block b sits at slots 64 (b mod 3) .. + 63, so block c + 1 lands on
// block c - 2, which chunk c + 1 no longer reads, and within a run a chunk
// builds only its own block -- c - 1 and c - 2 are the previous chunks' own.
//
// The 64 steps (64s, 64s + 64] of a chunk read, lane by lane, 127 consecutive
// members from block c - s - 1's first: base + lane - t.  Slots 192..255
// repeat slots 0..63 (a block with b mod 3 = 0 is written twice, by every
// lane: no divergence), so that such a read never wraps -- block c - s - 1 at
// 128 continues into the copy of block c - s at 192 -- and a step's slot needs
// no masking: one wave-uniform base per 64 steps.
//
// (A ring of 256 slots with slot = j & 255 and an 8-slot tail mirror was
// measured first: the wrap is a v_and per group and per look-ahead key, and
// with runs of one chunk the sweep was 3 % slower than the per-chunk ring.)
#ifndef ZS_SWEEP_RING_H
#define ZS_SWEEP_RING_H
#include <stdint.h>

#if defined(__HIPCC__)
#define ZS_SWR_FN static __host__ __device__ __forceinline__
#else
#define ZS_SWR_FN static inline
#endif

#define ZS_SWR_BLOCKS 3u       // blocks of 64 members in the ring
#define ZS_SWR_SLOTS 192u      // member slots per wave
#define ZS_SWR_MIRROR 64u      // slots ZS_SWR_SLOTS .. + 63 repeat slots 0..63
#define ZS_SWR_MAX_CHAIN 128u  // chain + 64 <= 192: three blocks read
#define ZS_SWR_RUN_DIV 32u     // a run is 1/32 of what is left (16 waves: half a wave's share)

// the first slot of block b (b >= -3: a block below member 0 holds zero records)
ZS_SWR_FN uint32_t zs_swr_block_slot(int32_t b) { return 64u * ((uint32_t)(b + 3) % ZS_SWR_BLOCKS); }

// block b is written a second time, ZS_SWR_SLOTS higher
ZS_SWR_FN int zs_swr_mirrored(int32_t b) { return zs_swr_block_slot(b) == 0u; }

// Chunk c, steps (64s, 64s + 64]: lane l reads step t at slot
// zs_swr_base(c, s) + l - t, in [0, 254].  A group of steps t0 .. t0 + n - 1 is
// read upwards from its lowest slot, that of step t0 + n - 1.
ZS_SWR_FN uint32_t zs_swr_base(int32_t c, uint32_t s) {
  return zs_swr_block_slot(c - (int32_t)s - 1) + 64u * s + 64u;
}

// after the sweep: the slot of member 64c + l - t, 1 <= t <= 128 + l (its position is read from the key)
ZS_SWR_FN uint32_t zs_swr_member_slot(int32_t c, uint32_t l, uint32_t t) {
  const uint32_t s = zs_swr_block_slot(c - 2) + 128u + l - t;
  return s >= ZS_SWR_SLOTS ? s - ZS_SWR_SLOTS : s;
}

// The blocks [lo, hi] whose records the ring holds, all written in the current
// run (wave-uniform; empty when lo > hi).  Nothing outside it is ever read.
typedef struct { int32_t lo, hi; } zs_swr_range;

ZS_SWR_FN zs_swr_range zs_swr_empty(void) {  // a run's start, or after a chunk that was skipped
  zs_swr_range r;
  r.lo = 1;
  r.hi = 0;
  return r;
}
ZS_SWR_FN int zs_swr_has(zs_swr_range r, int32_t b) { return r.lo <= b && b <= r.hi; }

// chunk c's own block is written: it takes the slots of block c - 3
ZS_SWR_FN zs_swr_range zs_swr_push(zs_swr_range r, int32_t c) {
  if (r.lo > r.hi || r.hi != c - 1) {  // nothing kept: the blocks before c are built again
    r.lo = c;
  } else if (r.lo < c - 2) {
    r.lo = c - 2;
  }
  r.hi = c;
  return r;
}
// block lo - 1 is written (the block before, or two before on demand)
ZS_SWR_FN zs_swr_range zs_swr_extend(zs_swr_range r, int32_t b) {
  r.lo = b;
  return r;
}

// chunks a wave claims at once with `left` unclaimed: guided self-scheduling.
// Only one workgroup fits a CU, so each workgroup's last chunks are exposed
// and the runs shrink to single chunks as the stream runs out.
ZS_SWR_FN uint32_t zs_swr_run_len(uint32_t left, uint32_t cap) {
  const uint32_t r = left / ZS_SWR_RUN_DIV;
  return r < 1u ? 1u : (r > cap ? cap : r);
}

// zs_k_sweep<true>'s condition on a level's chain budget: it and its quarter
// (the budget when prev_length >= good_match, deflate.ts:1075-1077) are
// multiples of 8 and at least 8.  The sweep's blocks are 64 steps and steps
// 1..8 are its opening group, so every later group is then exactly eight
// steps, t0 = 1 mod 8, and the quarter's snapshot falls on a group's end.
// (levels 5..9: 32, 128, 256, 1024, 4096; level 4's 16 / 4 does not qualify
// and takes zs_k_sweep<false>, whose groups are cut where they must be)
ZS_SWR_FN int zs_sweep_uniform8(int32_t chain) {
  return chain >= 8 && chain % 8 == 0 && (chain >> 2) >= 8 && (chain >> 2) % 8 == 0;
}

#endif
