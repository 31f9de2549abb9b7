// zs_sweep_ends.h -- when zs_k_sweep (deflate_sweep.hip, SwWave::ends) may keep
// the UNMASKED maximum of a group of eight chain steps in which some lane's
// chain ends.  Plain inline functions for the kernel and for the host model
// (tools/emu/emu_sweep_ends.c, tests/test_sweep_ends_model.py), which replays
// whole streams both ways -- every dead step's score zeroed, and this rule --
// and compares the lanes' state after every group.
//
// A step's score is its matched bits with the low three bits replaced by
// 7 - u, u its place in the group; a dead step (its key fails the liveness
// test) must score 0.  Liveness is monotone in the step, so a lane's dead steps
// are the last ones of its group, and the place tag makes an earlier step win a
// tie: the maximum gm of the unmasked scores is the masked maximum unless a
// dead step scores strictly more bytes than every live one.  With a0 = the lane
// is live when the group begins and last = it is live at the group's last step,
// a lane is settled -- the fold may take gm, 0 for a lane that is not in a0 --
// if one of these holds:
//   * !a0: the lane folds nothing;
//   * last: every step is live;
//   * gm does not raise the best (gm <= thr | 7) and is not long (gm < long_m):
//     the masked maximum is no larger, so it changes nothing either;
//   * gm is not long and the winner's step 7 - (gm & 7) is live: the masked
//     maximum is gm, and no step of the lane is long, so the long branch
//     visits nothing dead.
// The third case needs no key; the fourth reads the winner's key alone.  A wave
// with a lane that is not settled masks the group's scores step by step, as
// every such group did before, and takes the maximum again.  The lanes alive
// after the group are those of `last` either way.
#ifndef ZS_SWEEP_ENDS_H
#define ZS_SWEEP_ENDS_H
#include <stdint.h>

#if defined(__HIPCC__)
#define ZS_SWE_FN static __host__ __device__ __forceinline__
#else
#define ZS_SWE_FN static inline
#endif

// gm would replace the lane's best short candidate (thr = B << 3 | place)
ZS_SWE_FN int zs_swe_raises(uint32_t gm, uint32_t thr) { return gm > (thr | 7u); }

// gm is a long candidate: the long branch would visit the lane's steps
ZS_SWE_FN int zs_swe_long(uint32_t gm, uint32_t long_m) { return gm >= long_m; }

// the winner's key, counted in slots above the group's lowest (step u's record is at slot 7 - u)
ZS_SWE_FN uint32_t zs_swe_winner_slot(uint32_t gm) { return gm & 7u; }

// The winner's step is live, from its key wkey and the lane's chain limit
// klim.  head: the group opens the walk and its step 0 is the head candidate,
// which has its own rule (key >= khead) and is live for every lane of a0.
ZS_SWE_FN int zs_swe_winner_live(uint32_t gm, uint32_t wkey, uint32_t klim, int head) {
  return wkey > klim || (head && (gm & 7u) == 7u);
}

// the rule for one lane (win_live: zs_swe_winner_live; the wave reads the winners' keys when
// zs_swe_needs_key holds for one of its lanes)
ZS_SWE_FN int zs_swe_needs_key(int a0, int last, uint32_t gm, uint32_t thr) {
  return a0 && !last && zs_swe_raises(gm, thr);
}
ZS_SWE_FN int zs_swe_settled(int a0, int last, uint32_t gm, uint32_t thr, uint32_t long_m, int win_live) {
  if (!a0 || last) return 1;
  if (zs_swe_long(gm, long_m)) return 0;
  return !zs_swe_raises(gm, thr) || win_live;
}

#endif
