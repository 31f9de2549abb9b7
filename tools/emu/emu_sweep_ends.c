// emu_sweep_ends.c -- CPU model of how zs_k_sweep (deflate_sweep.hip, levels
// 5..9: SwWave::open8, run8, ends, remask) treats a group of eight chain steps
// in which some lane's chain ends.  It replays whole streams wave by wave (64
// members per chunk) and group by group, twice, each way with its own state:
//   A  every dead step's score is zeroed before the group's maximum is taken
//      (what every such group did before), and
//   B  the maximum of the unmasked scores is kept when zs_sweep_ends.h -- the
//      functions the kernel itself calls -- settles every lane of the wave,
//      else the wave masks as in A;
// and after every group the lanes' thr, bt, lthr, lbt, liveness and the
// chain >> 2 snapshots must be equal.  The scores are the kernel's, bit for
// bit: the record words of both signature forms, a zero record for a member in
// front of the window's first, xor + first differing bit + the place tag; a
// dead step is a member of another bucket, a member too far back, or a zero
// record, and scores whatever its record gives.  Long candidates are folded
// with zs_sweep_long.h as the kernel folds them (from the scores it is given).
// Test infrastructure (tests/test_sweep_ends_model.py); it checks the rule off
// the GPU, not the kernel binary (tests/test_gpu_sweep_ends.py does that).
//
// usage: emu_sweep_ends FILE CHAIN NICE [break]
//   FILE = u32 count, u32 sizes[count], bytes (streams of at most 65,537 bytes);
//   break: the winner's key is not looked at (the check must then fail).
// Prints mismatching lanes (the first few), and per chunk the groups behind the
// opening group -- fast, ends, of those with the winners' keys read and failed
// validation -- the opening groups with a partial lane, keys read and failed, and the
// lock-step steps, to set against the kernel's -DZS_SW_PROF=1 counters.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../zlib-streams-ts_amd/csrc/zs_sweep_long.h"
#include "../../zlib-streams-ts_amd/csrc/zs_sweep_ends.h"

#define MAXD 32506u
#define MAXN 65537u
static uint8_t buf[MAXN + 600];
static uint32_t cnt[32768], off[32768];
static uint16_t mem[65536];
static int a7, brk;

static uint32_t word(uint32_t q) { return buf[q] | buf[q + 1] << 8 | buf[q + 2] << 16 | (uint32_t)buf[q + 3] << 24; }
static uint32_t hash3(uint32_t w) { return (((w & 0xff) << 10) ^ (((w >> 8) & 0xff) << 5) ^ ((w >> 16) & 0xff)) & 0x7fff; }
static uint32_t x7(uint32_t w) {
  const uint32_t b0 = w & 0xff, b1 = (w >> 8) & 0xff;
  return ((b0 >> 5) & 3) | ((b1 & 7) << 2) | (((b1 >> 5) & 3) << 5);
}
typedef struct { uint32_t x, y, z, key; } rec_t;
static rec_t make_rec(uint32_t q) {  // SwSig<A7>::rec, SwWave::make_rec
  rec_t r;
  const uint32_t w0 = word(q);
  if (a7) { r.x = x7(w0) | (word(q + 3) << 8); r.y = word(q + 6); r.z = word(q + 10); }
  else { r.x = w0; r.y = word(q + 4); r.z = word(q + 8) & 0x00ffffffu; }
  r.key = (hash3(w0) << 16) | q;
  return r;
}
static uint32_t ffbl(uint32_t v) { return v ? (uint32_t)__builtin_ctz(v) : 0xffffffffu; }
static uint32_t addc(uint32_t a, uint32_t b) { return a > 0xffffffffu - b ? 0xffffffffu : a + b; }
static uint32_t min3(uint32_t a, uint32_t b, uint32_t c) { a = a < b ? a : b; return a < c ? a : c; }
// a step's score at place u: the lane's own record o against the candidate's r
static uint32_t score(const rec_t* o, const rec_t* r, uint32_t u) {
  uint32_t mb;
  if (a7) mb = min3(ffbl(r->x ^ o->x), addc(ffbl(r->y ^ o->y), 32), 64);
  else mb = min3(ffbl(r->x ^ o->x), addc(ffbl(r->y ^ o->y), 32), ffbl(r->z ^ (o->z | 0x01000000u)) + 64);
  return (mb & ~7u) | (7u - u);
}

typedef struct {
  uint32_t thr, bt, lthr, lbt, thr_s, bt_s, lthr_s, lbt_s;
  int alive, snapped;
} st_t;
typedef struct {  // what a lane keeps for the whole chunk
  int own;
  uint32_t p, maxc, nice, khead, klim, long_m;
  rec_t rown;
} lane_t;

static uint32_t lcp(uint32_t p, uint32_t q, uint32_t maxc) {
  uint32_t k = 0;
  while (k < maxc && buf[q + k] == buf[p + k]) k++;
  return k;
}
// SwWave::fold: gm and the scores sc the fold is given (steps t0 .. t0 + 7, qpos their members' positions)
static void fold(const lane_t* L, st_t* S, uint32_t gm, uint32_t t0, const uint32_t* sc, const uint32_t* qpos) {
  if (gm > (S->thr | 7u)) { S->thr = gm; S->bt = t0; }
  if (gm >= L->long_m && zs_swl_open(S->lthr, L->nice)) {
    uint32_t gl = 0;
    for (uint32_t u = 0; u < 8; u++)
      if (sc[u] >= L->long_m) gl = zs_swl_join(gl, zs_swl_score(lcp(L->p, qpos[u], L->maxc), L->maxc, L->nice, u));
    zs_swl_fold(gl, t0, &S->lthr, &S->lbt);
  }
}
static void snap(st_t* S) {
  S->thr_s = S->thr; S->bt_s = S->bt; S->lthr_s = S->lthr; S->lbt_s = S->lbt; S->snapped = 1;
}
static int same(const st_t* a, const st_t* b) {
  return a->thr == b->thr && a->bt == b->bt && a->lthr == b->lthr && a->lbt == b->lbt && a->alive == b->alive &&
         a->snapped == b->snapped &&
         (!a->snapped || (a->thr_s == b->thr_s && a->bt_s == b->bt_s && a->lthr_s == b->lthr_s && a->lbt_s == b->lbt_s));
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s FILE CHAIN NICE [break]\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  const uint32_t chain = (uint32_t)atoi(argv[2]), nice_cfg = (uint32_t)atoi(argv[3]), chain_s = chain >> 2;
  brk = argc > 4 && !strcmp(argv[4], "break");
  if (!f || chain < 32 || chain % 32) return 2;  // zs_sweep_uniform8: the budget and its quarter are multiples of 8
  uint32_t ns = 0, sizes[4096];
  if (fread(&ns, 4, 1, f) != 1 || ns > 4096 || fread(sizes, 4, ns, f) != ns) return 2;
  long bad = 0, groups = 0, chunks = 0, g_fast = 0, g_ends = 0, g_key = 0, g_fail = 0, o_part = 0, o_key = 0, o_fail = 0, steps = 0;
  long lanes_dead_winner = 0, lanes_long = 0;
  for (uint32_t si = 0; si < ns; si++) {
    const uint32_t n = sizes[si];
    if (n > MAXN) return 2;
    memset(buf, 0, sizeof buf);
    if (fread(buf, 1, n, f) != n) return 2;
    if (n < 3) continue;
    a7 = 1;
    for (uint32_t i = 0; i < n; i++) a7 &= buf[i] < 0x80;
    const uint32_t m = n - 2 < 65535u ? n - 2 : 65535u;  // (zs_plan.h: one window, its members the inserted positions)
    memset(cnt, 0, sizeof cnt);
    for (uint32_t p = 0; p < m; p++) cnt[hash3(word(p))]++;
    uint32_t run = 0;
    for (int h = 0; h < 32768; h++) { off[h] = run; run += cnt[h]; }
    for (uint32_t p = 0; p < m; p++) mem[off[hash3(word(p))]++] = (uint16_t)p;
    for (uint32_t c = 0; 64 * c < m; c++) {
      lane_t L[64];
      st_t A[64], B[64];
      chunks++;
      for (uint32_t i = 0; i < 64; i++) {  // SwWave::start
        const uint32_t k = 64 * c + i;
        lane_t* l = &L[i];
        memset(l, 0, sizeof *l);
        l->own = k < m;
        l->p = l->own ? mem[k] : 0;
        if (l->own) l->rown = make_rec(l->p);
        const uint32_t look = n - l->p, h = l->rown.key >> 16;
        l->maxc = look < 258 ? look : 258;
        l->nice = look < nice_cfg ? look : nice_cfg;
        l->long_m = l->maxc <= 12 ? 0xffffu : (a7 ? 64u : 88u);
        const uint32_t limit = l->p > MAXD ? l->p - MAXD : 0;
        l->khead = (h << 16) | (limit > 1 ? limit : 1);
        l->klim = (h << 16) | limit;
        st_t s0 = {a7 ? 7u : 23u, 0, ZS_SWL_NONE, 0, a7 ? 7u : 23u, 0, ZS_SWL_NONE, 0, 0, 0};
        A[i] = B[i] = s0;
      }
      for (uint32_t t0 = 1; t0 <= chain; t0 += 8) {
        const int head = t0 == 1;
        uint32_t sc[64][8], qpos[64][8], key[64][8];
        int live[64][8], a0[64], last[64], any = 0, part = 0;
        for (uint32_t i = 0; i < 64; i++) {
          for (uint32_t u = 0; u < 8; u++) {
            const long j = (long)(64 * c + i) - (long)(t0 + u);
            rec_t r = {0, 0, 0, 0};  // a member in front of the first: key 0 fails every liveness test
            if (j >= 0 && (uint32_t)j < m) r = make_rec(mem[j]);
            sc[i][u] = score(&L[i].rown, &r, u);
            qpos[i][u] = r.key & 0xffffu;
            key[i][u] = r.key;
            live[i][u] = head && u == 0 ? L[i].own && r.key >= L[i].khead
                                        : (u ? live[i][u - 1] : A[i].alive) && r.key > L[i].klim;
          }
          a0[i] = head ? live[i][0] : A[i].alive;
          last[i] = live[i][7];
          any |= a0[i];
          part |= a0[i] && !last[i];
        }
        if (!any) break;  // no lane of the wave is alive: the walk ends
        groups++;
        steps += 8;
        if (head) o_part += part; else if (part) g_ends++; else g_fast++;
        // A: masked
        for (uint32_t i = 0; i < 64; i++) {
          uint32_t ms[8], gm = 0;
          for (uint32_t u = 0; u < 8; u++) { ms[u] = live[i][u] ? sc[i][u] : 0; gm = ms[u] > gm ? ms[u] : gm; }
          fold(&L[i], &A[i], a0[i] ? gm : 0, t0, ms, qpos[i]);
          A[i].alive = last[i];
        }
        // B: unmasked, validated
        int unsettled = 0, keyread = 0;
        uint32_t gmu[64];
        for (uint32_t i = 0; i < 64; i++) {
          uint32_t gm = 0;
          for (uint32_t u = 0; u < 8; u++) gm = sc[i][u] > gm ? sc[i][u] : gm;
          gmu[i] = a0[i] ? gm : 0;
        }
        if (part) {
          for (uint32_t i = 0; i < 64; i++)
            keyread |= zs_swe_needs_key(a0[i], last[i], gmu[i], B[i].thr);
          for (uint32_t i = 0; i < 64; i++) {
            const uint32_t wk = key[i][7u - zs_swe_winner_slot(gmu[i])];
            const int wl = brk ? 1 : zs_swe_winner_live(gmu[i], wk, L[i].klim, head);
            if (!zs_swe_settled(a0[i], last[i], gmu[i], B[i].thr, L[i].long_m, wl)) {
              unsettled = 1;
              if (zs_swe_long(gmu[i], L[i].long_m)) lanes_long++; else lanes_dead_winner++;
            }
          }
          if (head) { o_key += keyread; o_fail += unsettled; } else { g_key += keyread; g_fail += unsettled; }
        }
        for (uint32_t i = 0; i < 64; i++) {
          if (unsettled) {
            uint32_t ms[8], gm = 0;
            for (uint32_t u = 0; u < 8; u++) { ms[u] = live[i][u] ? sc[i][u] : 0; gm = ms[u] > gm ? ms[u] : gm; }
            fold(&L[i], &B[i], a0[i] ? gm : 0, t0, ms, qpos[i]);
          } else {
            fold(&L[i], &B[i], gmu[i], t0, sc[i], qpos[i]);
          }
          B[i].alive = last[i];
        }
        for (uint32_t i = 0; i < 64; i++) {
          if (t0 + 7 == chain_s) { snap(&A[i]); snap(&B[i]); }
          if (!same(&A[i], &B[i])) {
            if (bad < 10)
              printf("stream %u chunk %u lane %u steps %u..%u: masked thr %u bt %u lthr %u lbt %u, rule thr %u bt %u lthr %u "
                     "lbt %u\n", si, c, i, t0, t0 + 7, A[i].thr, A[i].bt, A[i].lthr, A[i].lbt, B[i].thr, B[i].bt, B[i].lthr,
                     B[i].lbt);
            bad++;
            B[i] = A[i];  // (one report per divergence)
          }
        }
      }
    }
  }
  const double ch = chunks ? (double)chunks : 1.0;
  printf("chunks %ld, groups %ld, mismatches %ld\n", chunks, groups, bad);
  printf("per chunk behind the opening group: fast %.2f, ends %.2f (keys read %.2f, failed %.2f); opening group: "
         "partial %.2f, keys read %.2f, failed %.2f; lock-step steps %.1f\n", g_fast / ch, g_ends / ch, g_key / ch, g_fail / ch,
         o_part / ch, o_key / ch, o_fail / ch, steps / ch);
  printf("unsettled lanes: dead winner %ld, long %ld\n", lanes_dead_winner, lanes_long);
  return bad != 0;
}
