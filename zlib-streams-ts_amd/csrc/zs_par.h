// zs_par.h -- how deflateInit2_'s windowBits and memLevel (deflate.ts:253-343) reach the
// deflate kernels without touching the instances every plain call launches.
//
// deflate_match.hip, deflate_parse.hip, deflate_fast.hip and deflate_emit.hip are each compiled
// TWICE (Makefile).  The plain build sees the macros below as the constants the kernels always
// had -- 32 KiB window, 15-bit hash, 16,383 symbols per block -- and as nothing where an argument
// would be: after preprocessing its source is what it was before the parameters existed, so its
// code is too (a translation unit of its own: not even the inliner sees a second caller).  The
// build with ZS_PAR_BUILD renames the kernels to *_par, gives them one more argument, the
// zs_kpar `kp`, and reads the values from it.  The branch-free parse step (zs_parse.h:19-21)
// thus carries no runtime parameter for anyone who did not ask for one.
//
//   ZS_PN(name)        the kernel's name (name / name_par)
//   ZS_PAR_ARG         the extra parameter in a parameter list (nothing / , zs_kpar kp)
//   ZS_PAR_TYPE        ... in an explicit instantiation (nothing / , zs_kpar)
//   ZS_PAR_PASS        ... passed on to a helper (nothing / , kp)
//   ZS_P_W             w_size: the slide step, prev[]'s entries       (32768u)
//   ZS_P_W_ULL         ... as a 64-bit value                           (32768ull)
//   ZS_P_WMASK         w_size - 1                                      (0x7fffu)
//   ZS_P_2W            the window, 2 w_size                            (65536u)
//   ZS_P_MAX_DIST      w_size - 262                                    (ZS_MAX_DIST)
//   ZS_P_SLIDE_AT      2 w_size - 262: fill_window slides from here    (ZS_SLIDE_AT)
//   ZS_P_SYM_END       lit_bufsize - 1                                 (ZS_SYM_END)
//   ZS_P_HSHIFT / ZS_P_HMASK, ZS_P_HASHW(w): the hash of the low three bytes of w.  3 x shift >=
//                      hash_bits, so three UPDATE_HASH steps (deflate.ts:109-111) leave nothing
//                      of the bytes before and the closed form holds for every memLevel
#pragma once
#include "zs_common.h"

#ifndef ZS_PAR_BUILD
#define ZS_PAR_BUILD 0
#endif

#if ZS_PAR_BUILD
#define ZS_PN(name) name##_par
#define ZS_PAR_ARG , zs_kpar kp
#define ZS_PAR_TYPE , zs_kpar
#define ZS_PAR_PASS , kp
#define ZS_P_W kp.w_size
#define ZS_P_W_ULL (uint64_t)kp.w_size
#define ZS_P_WMASK (kp.w_size - 1u)
#define ZS_P_2W (2u * kp.w_size)
#define ZS_P_MAX_DIST (kp.w_size - ZS_MIN_LOOKAHEAD)
#define ZS_P_SLIDE_AT (2u * kp.w_size - ZS_MIN_LOOKAHEAD)
#define ZS_P_SYM_END kp.sym_end
#define ZS_P_HSHIFT kp.hash_shift
#define ZS_P_HMASK kp.hash_mask
#define ZS_P_HASHW(w) \
  (((((w) & 0xffu) << (2u * kp.hash_shift)) ^ ((((w) >> 8) & 0xffu) << kp.hash_shift) ^ (((w) >> 16) & 0xffu)) & kp.hash_mask)
#else
#define ZS_PN(name) name
#define ZS_PAR_ARG
#define ZS_PAR_TYPE
#define ZS_PAR_PASS
#define ZS_P_W 32768u
#define ZS_P_W_ULL 32768ull
#define ZS_P_WMASK 0x7fffu
#define ZS_P_2W 65536u
#define ZS_P_MAX_DIST ZS_MAX_DIST
#define ZS_P_SLIDE_AT ZS_SLIDE_AT
#define ZS_P_SYM_END ZS_SYM_END
#define ZS_P_HSHIFT 5
#define ZS_P_HMASK ZS_HASH_MASK
#define ZS_P_HASHW(w) (((((w) & 0xffu) << 10) ^ ((((w) >> 8) & 0xffu) << 5) ^ (((w) >> 16) & 0xffu)) & ZS_HASH_MASK)
#endif
