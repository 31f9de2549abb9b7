// sweep_long_model.c -- CPU model of where zs_k_sweep (deflate_sweep.hip) meets
// LONG candidates: a bucket sort of every stream's positions by (hash,
// position) and the lock-step walk of its 64-member chunks in the kernel's
// groups of steps (steps 1..8 as one group where chain >> 2 >= 8, else the head
// and 2..4; then eights cut at chain >> 2 and at 64-step blocks; with `pieces`,
// the head, 2..4 and eights from step 5 at every level, as before the opening group).  Counts, per group,
// each lane's long candidates (lcp >= 10 -- the whole 7-bit signature -- and
// >= 14, >= 18: the ring's extension bytes do not settle them, the extension
// loop's second round) and the most long candidates any lane has in the group.
//   sweep_long_model FILE [chain [pieces]]    FILE: 64 KiB streams back to back
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAXD 32506u
#define SB 65536u
static uint8_t buf[SB + 300];
static uint32_t cnt[32768], off[32768], st[32768], hh[SB];
static uint16_t mem[SB];

static uint32_t lcp(uint32_t p, uint32_t q, uint32_t maxc) {
  uint32_t k = 0;
  while (k < maxc && buf[p + k] == buf[q + k]) k++;
  return k;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const uint32_t chain = argc > 2 ? (uint32_t)atoi(argv[2]) : 128u, bs = chain >> 2;
  const int open8 = !(argc > 3 && !strcmp(argv[3], "pieces")) && bs >= 8;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  double streams = 0, chunks = 0, groups = 0, wsteps = 0, exact = 0, cands = 0;
  double lgroups = 0, l10 = 0, l14 = 0, l18 = 0, most[4] = {0, 0, 0, 0};
  while (fread(buf, 1, SB, f) == SB) {
    const uint32_t n = SB, m = n - 2;
    streams++;
    memset(cnt, 0, sizeof cnt);
    for (uint32_t p = 0; p < m; p++) {
      hh[p] = ((buf[p] << 10) ^ (buf[p + 1] << 5) ^ buf[p + 2]) & 0x7fff;
      cnt[hh[p]]++;
    }
    uint32_t r = 0;
    for (int h = 0; h < 32768; h++) { off[h] = r; r += cnt[h]; }
    memcpy(st, off, sizeof st);
    for (uint32_t p = 0; p < m; p++) mem[st[hh[p]]++] = (uint16_t)p;
    for (uint32_t c = 0; c < m; c += 64) {
      // the live steps of the chunk's lanes (liveness is monotone in t)
      uint32_t live[64], mx = 0;
      for (uint32_t i = 0; i < 64; i++) {
        live[i] = 0;
        const uint32_t k = c + i;
        if (k >= m) continue;
        const uint32_t p = mem[k], h = hh[p], lim = p > MAXD ? p - MAXD : 0;
        for (uint32_t t = 1; t <= chain; t++) {
          const int j = (int)k - (int)t;
          if (j < (int)off[h]) break;
          const uint32_t q = mem[j];
          if (t == 1 ? q < (lim > 1 ? lim : 1) : q <= lim) break;
          live[i] = t;
        }
        exact += live[i];
        if (live[i] > mx) mx = live[i];
      }
      chunks++;
      // the groups, as long as a lane is live
      uint32_t t0 = 1;
      while (t0 <= mx) {
        uint32_t t1;
        if (open8 && t0 == 1) t1 = 8;
        else if (t0 == 1) t1 = 1;
        else if (t0 == 2) t1 = 4;
        else {
          const uint32_t tb = ((t0 - 1) / 64 + 1) * 64 < chain ? ((t0 - 1) / 64 + 1) * 64 : chain;
          t1 = t0 + 7 <= tb ? t0 + 7 : t0 + 3;
          if (t0 <= bs && t1 > bs) t1 = bs;
        }
        groups++;
        wsteps += t1 - t0 + 1;
        uint32_t gmost = 0;
        for (uint32_t i = 0; i < 64; i++) {
          const uint32_t k = c + i;
          if (k >= m) continue;
          const uint32_t p = mem[k], maxc = n - p < 258 ? n - p : 258;
          uint32_t mine = 0;
          for (uint32_t t = t0; t <= t1 && t <= live[i]; t++) {
            cands++;
            if (maxc <= 12) continue;  // the last positions are walked exactly after the sweep
            const uint32_t l = lcp(p, mem[k - t], maxc);
            if (l >= 10) { l10++; mine++; }
            if (l >= 14) l14++;
            if (l >= 18) l18++;
          }
          if (mine > gmost) gmost = mine;
        }
        if (gmost) {
          lgroups++;
          most[gmost > 3 ? 3 : gmost]++;
        }
        t0 = t1 + 1;
      }
    }
  }
  printf("chain %u%s, %.0f streams of 64 KiB, %.0f chunks\n", chain, open8 ? ", steps 1..8 one group" : ", head | 2..4 | from 5", streams, chunks);
  printf("per chunk: groups %.2f  lock-step steps %.1f  exact steps per position %.1f  candidate compares %.0f\n", groups / chunks,
         wsteps / chunks, exact / (streams * (SB - 2)), cands / chunks);
  printf("per chunk: groups holding a long candidate %.2f  long candidates %.2f\n", lgroups / chunks, l10 / chunks);
  printf("long groups by the most long candidates of one lane: one %.1f %%  two %.1f %%  three or more %.1f %%\n",
         100 * most[1] / lgroups, 100 * most[2] / lgroups, 100 * most[3] / lgroups);
  printf("long candidates matching >= 14 bytes %.1f %%  >= 18 bytes %.1f %%\n", 100 * l14 / l10, 100 * l18 / l10);
  return 0;
}
