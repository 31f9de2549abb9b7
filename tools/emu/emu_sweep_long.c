// emu_sweep_long.c -- host check of csrc/zs_sweep_long.h, the rule by which
// zs_k_sweep's fold picks among the long candidates of a group of eight chain
// steps, against the reference's serial walk (deflate.ts:1082-1105: the first
// strictly longer candidate, the walk ends at the first one of >= nice bytes).
//
// For every nice in {16, 32, 128, 258}, maxc in {13, 14, 258}, incoming best
// (none, shorter than, equal to and longer than the group's candidates, at nice
// and above it) and all 256 masks of long steps, with the steps' lengths from
// {10, 11, 13, 14, nice - 1, nice, nice + 1, 258}: every assignment for masks
// of up to three steps, 256 drawn ones for the others.  Both forms the kernel
// uses are replayed: every long step joined in turn, and the first long step
// taken from the group's maximum score with the rest joined afterwards.
//   emu_sweep_long          check
//   emu_sweep_long break    the same with the nice cap left out (must fail)
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../zlib-streams-ts_amd/csrc/zs_sweep_long.h"

#define LONG_SCORE 64u  // a long step's matched bits (the 7-bit form; the 11-byte form has 88)

static uint32_t rng = 12345u;
static uint32_t rnd(void) {
  rng ^= rng << 13;
  rng ^= rng >> 17;
  rng ^= rng << 5;
  return rng;
}

static int brk = 0;
static unsigned long long cases = 0, bad = 0;

static void one(uint32_t nice, uint32_t maxc, uint32_t mask, const uint32_t* lcp, uint32_t in_len, uint32_t t0) {
  const uint32_t in_step = in_len ? 3u : 0u;
  // the serial walk, entered with the best of the steps before the group
  uint32_t bl = in_len < maxc ? in_len : maxc, bs = in_step;
  int ended = in_len && bl >= nice;
  for (uint32_t u = 0; u < 8 && !ended; u++) {
    if (!((mask >> u) & 1u)) continue;
    const uint32_t len = lcp[u] < maxc ? lcp[u] : maxc;
    if (len > bl) {
      bl = len;
      bs = t0 + u;
      if (len >= nice) ended = 1;
    }
  }
  const uint32_t want_len = bl < nice ? bl : nice, want_step = bs;
  // the kernel's state: the length capped at nice
  const uint32_t nice_k = brk ? 0xffffu : nice;
  uint32_t l0 = in_len < maxc ? in_len : maxc;
  l0 = l0 < nice ? l0 : nice;
  const uint32_t lthr0 = in_len ? (l0 << 3) | 7u : ZS_SWL_NONE;
  // the steps' scores and the group's maximum
  uint32_t sc[8], gm = 0;
  for (uint32_t u = 0; u < 8; u++) {
    sc[u] = (((mask >> u) & 1u) ? LONG_SCORE : 8u * (rnd() % (LONG_SCORE / 8u))) | (7u - u);
    gm = gm > sc[u] ? gm : sc[u];
  }
  for (int form = 0; form < 2; form++) {
    uint32_t lthr = lthr0, lbt = in_step;
    if (gm >= LONG_SCORE && zs_swl_open(lthr, nice)) {
      uint32_t gl = 0, lm = mask;
      if (form == 1) {  // the first long step from the maximum, the others afterwards
        const uint32_t u1 = zs_swl_first(gm);
        if (!((mask >> u1) & 1u) || (mask & ((1u << u1) - 1u))) {
          bad++;
          continue;
        }
        gl = zs_swl_score(lcp[u1], maxc, nice_k, u1);
        lm &= ~(1u << u1);
      }
      while (lm) {
        const uint32_t u = (uint32_t)__builtin_ctz(lm);
        lm &= lm - 1u;
        gl = zs_swl_join(gl, zs_swl_score(lcp[u], maxc, nice_k, u));
      }
      zs_swl_fold(gl, t0, &lthr, &lbt);
    }
    cases++;
    const uint32_t got_len = lthr >> 3;
    if (got_len != want_len || lbt != want_step || (lthr & 7u) != 7u) {
      if (bad < 10)
        printf("nice %u maxc %u mask %02x in %u form %d: got len %u step %u, want len %u step %u\n", nice, maxc, mask,
               in_len, form, got_len, lbt, want_len, want_step);
      bad++;
    }
  }
}

int main(int argc, char** argv) {
  brk = argc > 1 && !strcmp(argv[1], "break");
  static const uint32_t nices[4] = {16, 32, 128, 258}, maxcs[3] = {13, 14, 258};
  for (int ni = 0; ni < 4; ni++)
    for (int mi = 0; mi < 3; mi++) {
      const uint32_t nice = nices[ni], maxc = maxcs[mi];
      const uint32_t lens[8] = {10, 11, 13, 14, nice - 1, nice, nice + 1, 258};
      const uint32_t ins[9] = {0, 10, 12, 13, 14, nice - 1, nice, nice + 1, 258};
      for (int ii = 0; ii < 9; ii++)
        for (uint32_t mask = 0; mask < 256; mask++) {
          uint32_t at[8], k = 0, lcp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          for (uint32_t u = 0; u < 8; u++)
            if ((mask >> u) & 1u) at[k++] = u;
          const uint32_t t0 = 8u * (1u + mask % 15u) + 1u;
          if (k <= 3) {
            uint32_t total = 1;
            for (uint32_t j = 0; j < k; j++) total *= 8;
            for (uint32_t a = 0; a < total; a++) {
              for (uint32_t j = 0, x = a; j < k; j++, x /= 8) lcp[at[j]] = lens[x % 8];
              one(nice, maxc, mask, lcp, ins[ii], t0);
            }
          } else {
            for (uint32_t a = 0; a < 256; a++) {
              for (uint32_t j = 0; j < k; j++) lcp[at[j]] = lens[rnd() % 8];
              one(nice, maxc, mask, lcp, ins[ii], t0);
            }
          }
        }
    }
  printf("cases %llu, bad %llu\n", cases, bad);
  return bad ? 1 : 0;
}
