// zs_sweep_long.h -- how zs_k_sweep (deflate_sweep.hip, fold) chooses among a
// group's LONG candidates: chain steps whose whole signature matches and whose
// exact length comes from the window.  Plain inline functions for the kernel
// and for the host check (tools/emu/emu_sweep_long.c,
// tests/test_sweep_long_model.py), which compares them with the reference's
// serial walk (deflate.ts:1082-1105).
//
// The walk keeps the first strictly longer candidate and ends at the first one
// of at least `nice` bytes.  A lane's best long candidate is lthr = len << 3 | 7
// (7: no candidate yet, len 0) with its chain step lbt (0: none).  A candidate
// of the group at place u (0..7, step t0 + u) scores len' << 3 | (7 - u) with
// len' = min(len, maxc, nice): the maximum of a group's scores is its longest
// candidate and, among equally long ones, the earliest.  Capping at nice makes
// the first nice candidate tie with every later one, so it stays first, as if
// the walk had ended there; a lane whose best has reached nice takes no more
// candidates (zs_swl_open).  The group's winner replaces the best only when
// strictly longer.  (The true length of a capped winner is measured once,
// after the sweep.)
#ifndef ZS_SWEEP_LONG_H
#define ZS_SWEEP_LONG_H
#include <stdint.h>

#if defined(__HIPCC__)
#define ZS_SWL_FN static __host__ __device__ __forceinline__
#else
#define ZS_SWL_FN static inline
#endif

#define ZS_SWL_NONE 7u  // lthr of a lane without a long candidate

// the walk has not ended: the best so far is shorter than nice
ZS_SWL_FN int zs_swl_open(uint32_t lthr, uint32_t nice) { return (lthr >> 3) < nice; }

// the score of the candidate at place u of its group, len = its matched bytes
ZS_SWL_FN uint32_t zs_swl_score(uint32_t len, uint32_t maxc, uint32_t nice, uint32_t u) {
  uint32_t l = len < maxc ? len : maxc;
  l = l < nice ? l : nice;
  return (l << 3) | (7u - u);
}

// the group's candidates so far (gl, 0: none) and one more
ZS_SWL_FN uint32_t zs_swl_join(uint32_t gl, uint32_t score) { return gl > score ? gl : score; }

// the group's winner gl (steps from t0) against the lane's best
ZS_SWL_FN void zs_swl_fold(uint32_t gl, uint32_t t0, uint32_t* lthr, uint32_t* lbt) {
  const int up = gl > *lthr;  // strictly longer: lthr's low bits are 7
  *lbt = up ? t0 + 7u - (gl & 7u) : *lbt;
  *lthr = up ? (gl | 7u) : *lthr;
}

// The place of a group's first long candidate, from the maximum gm of the
// group's step scores (matched bits & ~7 | 7 - place; long steps score at or
// above the form's LONG, short ones below): the first long step is the maximum.
ZS_SWL_FN uint32_t zs_swl_first(uint32_t gm) { return 7u - (gm & 7u); }

#endif
