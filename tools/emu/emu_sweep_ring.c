// emu_sweep_ring.c -- replays the writes and reads of zs_k_sweep's persistent
// per-wave ring (deflate_sweep.hip, levels 4..6) with the arithmetic of
// csrc/zs_sweep_ring.h, the header the kernel itself uses.
//
//   emu_sweep_ring M [break]
//
// For M members it runs every combination of chain (16, 32, 128), run cap
// (1, 2, 8, 16), skipped-chunk pattern (none, the first chunks, the last chunks,
// alternating) and "the sweep goes past step 64" pattern (never, always,
// alternating): 16 waves claim runs from a shared counter in turn, and each
// wave does per chunk what sw_body<., ., true> does to its ring -- push the
// own block, build the block before where the range lacks it, build the block
// two before on demand -- and then every read of the chunk: the head, steps
// 2..4, the groups of 8 and 4 upwards from their lowest slot (through the
// mirror of slots 0..63 at 192..255), the look-ahead keys and the member()
// reads after the sweep.  Each read must find the member the
// step means, written in the wave's current run.
//
// "break" (the test of the test) leaves the mirror unwritten, which must be
// reported as bad reads.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../zlib-streams-ts_amd/csrc/zs_sweep_ring.h"

#define WAVES 16
#define NSLOT (ZS_SWR_SLOTS + ZS_SWR_MIRROR)

typedef struct {
  int32_t member[NSLOT];  // the member whose record the slot holds
  uint32_t run[NSLOT];    // the run that wrote it (0: never)
  zs_swr_range vr;
  uint32_t c, ce, cur_run;
  int fresh;
} wave_t;

static int g_break_mirror;
static unsigned long long g_reads, g_bad, g_builds;
static uint32_t g_next, g_run_id;

static void build_block(wave_t* w, int32_t b) {  // SwRingP::put for the 64 lanes
  g_builds++;
  for (int lane = 0; lane < 64; lane++) {
    const int32_t j = 64 * b + lane;
    const uint32_t s = zs_swr_block_slot(b) + (uint32_t)lane;
    w->member[s] = j;
    w->run[s] = w->cur_run;
    if (zs_swr_mirrored(b) && !g_break_mirror) {
      w->member[s + ZS_SWR_SLOTS] = j;
      w->run[s + ZS_SWR_SLOTS] = w->cur_run;
    }
  }
}

static void check(const wave_t* w, uint32_t slot, int32_t want, const char* what, uint32_t t) {
  g_reads++;
  if (slot >= NSLOT || w->member[slot] != want || w->run[slot] != w->cur_run) {
    if (g_bad++ < 5)
      fprintf(stderr, "  %s step %u: slot %u holds member %d of run %u, wanted member %d of run %u\n", what, t, slot,
              slot < NSLOT ? w->member[slot] : -1, slot < NSLOT ? w->run[slot] : 0u, want, w->cur_run);
  }
}

// SwWave::run(): steps [ta, tb] in groups of 8, or 4 where the range or the chain >> 2 snapshot cuts them
static void sweep_range(const wave_t* w, int32_t k, uint32_t base, uint32_t ta, uint32_t tb, uint32_t budget_s) {
  for (uint32_t t0 = ta; t0 <= tb;) {
    uint32_t t1 = t0 + 7u <= tb ? t0 + 7u : t0 + 3u;
    if (t0 <= budget_s && t1 > budget_s) t1 = budget_s;
    const uint32_t n = t1 - t0 + 1u;
    check(w, base - t1, k - (int32_t)t1, "look-ahead key", t1);
    const uint32_t lo = base - t0 - (n - 1u);
    for (uint32_t u = 0; u < n; u++) {
      check(w, lo + (n - 1u - u), k - (int32_t)(t0 + u), "group", t0 + u);
      check(w, base - t0 - u, k - (int32_t)(t0 + u), "long candidate", t0 + u);
    }
    t0 = t1 + 1u;
  }
}

static void claim_run(wave_t* w, uint32_t nchunks, uint32_t cap) {
  const uint32_t r = zs_swr_run_len(g_next < nchunks ? nchunks - g_next : 0u, cap);
  w->c = g_next;
  g_next += r;
  w->ce = w->c + r < nchunks ? w->c + r : nchunks;
  w->fresh = 1;
}

static int skipped(int pat, uint32_t c, uint32_t nchunks) {
  switch (pat) {
    case 1: return c < (nchunks + 1) / 2;   // the look-back half of a later window of zeros
    case 2: return c >= nchunks - (nchunks + 2) / 3;
    case 3: return (c & 1u) != 0;
    case 4: return (c % 3u) == 1u;
    default: return 0;
  }
}
static int past64(int pat, uint32_t c) { return pat == 0 ? 0 : pat == 1 ? 1 : pat == 2 ? (int)(c & 1u) : (int)((c >> 1) & 1u); }

static void chunk(wave_t* w, uint32_t c, uint32_t chain, int skip, int deep) {
  if (w->fresh) {
    w->cur_run = ++g_run_id;
    w->vr = zs_swr_empty();
    w->fresh = 0;
  }
  if (skip) {  // no own lane: nothing is built and the range breaks
    w->vr = zs_swr_empty();
    return;
  }
  const int32_t cc = (int32_t)c;
  build_block(w, cc);
  w->vr = zs_swr_push(w->vr, cc);
  if (!zs_swr_has(w->vr, cc - 1)) {
    build_block(w, cc - 1);
    w->vr = zs_swr_extend(w->vr, cc - 1);
  }
  const uint32_t budget_s = chain >> 2;
  for (int lane = 0; lane < 64; lane++) {
    const int32_t k = 64 * cc + lane;
    const uint32_t base0 = zs_swr_base(cc, 0u) + (uint32_t)lane;
    check(w, base0 - 1u, k - 1, "head", 1u);
    if (chain >= 4u)
      for (uint32_t u = 0; u < 3u; u++) check(w, base0 - 2u - u, k - 2 - (int32_t)u, "masked", 2u + u);
  }
  for (uint32_t b = 0; chain > 4u; b++) {
    if (b >= 1u) {
      if (!deep) break;  // every chain ended within the block
      if (!zs_swr_has(w->vr, cc - (int32_t)b - 1)) {
        build_block(w, cc - (int32_t)b - 1);
        w->vr = zs_swr_extend(w->vr, cc - (int32_t)b - 1);
      }
    }
    const uint32_t ta = b == 0 ? 5u : 64u * b + 1u;
    const uint32_t tb = 64u * b + 64u < chain ? 64u * b + 64u : chain;
    for (int lane = 0; lane < 64; lane++) sweep_range(w, 64 * cc + lane, zs_swr_base(cc, b) + (uint32_t)lane, ta, tb, budget_s);
    if (tb >= chain) break;
  }
  // after the sweep: member(k - t) for a step that was swept (the tail re-walk reads them all)
  const uint32_t swept = chain <= 64u || deep ? chain : 64u;
  for (int lane = 0; lane < 64; lane++)
    for (uint32_t t = 1; t <= swept; t++)
      check(w, zs_swr_member_slot(cc, (uint32_t)lane, t), 64 * cc + lane - (int32_t)t, "member", t);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s M [break]\n", argv[0]);
    return 2;
  }
  const uint32_t m = (uint32_t)strtoul(argv[1], 0, 10);
  g_break_mirror = argc > 2 && !strcmp(argv[2], "break");
  const uint32_t nchunks = (m + 63u) / 64u;
  static const uint32_t chains[] = {16, 32, 128}, caps[] = {1, 2, 8, 16};
  static wave_t W[WAVES];
  unsigned long long cases = 0, bad_cases = 0;
  for (int ci = 0; ci < 3; ci++)
    for (int ki = 0; ki < 4; ki++)
      for (int sp = 0; sp < 5; sp++)
        for (int pp = 0; pp < 4; pp++) {
          memset(W, 0, sizeof(W));
          g_next = 0;
          g_run_id = 0;
          const unsigned long long bad0 = g_bad;
          uint32_t done = 0;
          for (int w = 0; w < WAVES; w++) {
            W[w].vr = zs_swr_empty();
            claim_run(&W[w], nchunks, caps[ki]);
          }
          // the waves take turns, one chunk each; wave w sits out every (w + 2)-th turn so that the runs interleave
          for (uint32_t turn = 0; done < WAVES; turn++) {
            done = 0;
            for (int w = 0; w < WAVES; w++) {
              wave_t* x = &W[w];
              if (x->c >= nchunks) { done++; continue; }
              if (turn % (uint32_t)(w + 2) == 0) continue;
              chunk(x, x->c, chains[ci], skipped(sp, x->c, nchunks), past64(pp, x->c));
              if (++x->c >= x->ce) claim_run(x, nchunks, caps[ki]);
            }
          }
          cases++;
          if (g_bad != bad0) {
            bad_cases++;
            if (bad_cases <= 3) fprintf(stderr, "m %u chain %u cap %u skip %d past64 %d: bad reads\n", m, chains[ci], caps[ki], sp, pp);
          }
        }
  printf("m %u: %llu cases, %llu reads, %llu blocks built, bad reads %llu in %llu cases\n", m, cases, g_reads, g_builds, g_bad,
         bad_cases);
  return g_bad ? 1 : 0;
}
