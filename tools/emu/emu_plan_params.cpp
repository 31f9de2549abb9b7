// emu_plan_params.cpp -- what csrc/zs_plan.h decides for deflateInit2_'s windowBits and
// memLevel (zs_make_params, zs_plan_deflate's route and block counts, zs_plan_fast_params'
// table of kernel instances), printed one line of key=value pairs per case for
// tests/test_plan_params.py.  Plain C++, no ROCm headers.
//   g++ -std=c++17 -O2 -o emu_plan_params tools/emu/emu_plan_params.cpp && ./emu_plan_params
// With -DEMU_PLAN_BEFORE the program uses only what zs_plan.h had before the parameters
// existed and prints the "default/..." lines alone: compiled against that header it gave
// the figures the test pins the default plan to.
#include <stdio.h>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"

static const uint32_t kLens[] = {0, 1, 100, 16383, 65537, 65538, 200000};
static const uint32_t kN = 7;

// the plan of a batch without dictionaries at `level`, parameters q (both levels 1..3 options on)
static void plan(const zs_route_opts& o, int level, const zs_deflate_params& q, zs_deflate_plan& p) {
  zs_deflate_req r;
  r.level = level;
  r.q = q;
  zs_plan_deflate(r, o, true, true, kN, kLens, nullptr, 0, p);
}

static void print_plan(const char* name, const zs_deflate_plan& p, uint32_t n) {
  uint64_t pos = 0, blk = 0, seg = 0;
  for (uint32_t i = 0; i < n; i++) {
    pos = pos * 31 + p.pos[i];
    blk = blk * 31 + p.blk[i];
  }
  for (const zs_sweep_seg& s : p.segs) seg = seg * 31 + s.s + 3ull * s.base + 5ull * s.olo + 7ull * s.ohi + 11ull * s.mb;
  printf("case=%s P=%llu members=%llu B=%u max_len=%u max_blk=%u pw=%d nseg=%zu prevd=%zu mres=%zu syms=%zu pscr=%zu "
         "codes=%zu hdr=%zu pos=%llu blk=%llu seg=%llu\n",
         name, (unsigned long long)p.P, (unsigned long long)p.members, p.B, p.max_len, p.max_blk, p.pw, p.segs.size(),
         p.prevd_bytes, p.mres_bytes, p.syms_bytes, p.pscr_bytes, p.codes_bytes, p.hdr_bytes, (unsigned long long)pos,
         (unsigned long long)blk, (unsigned long long)seg);
}

int main() {
  char name[64];
  for (int sweep = 0; sweep <= 1; sweep++)
    for (int level : {1, 6}) {
      zs_route_opts o;
      o.match_sweep = sweep != 0;
      zs_deflate_plan p;
      plan(o, level, zs_deflate_params(), p);  // as every plain entry calls it
      snprintf(name, sizeof name, "default/s%d/l%d", sweep, level);
      print_plan(name, p, kN);
#ifndef EMU_PLAN_BEFORE
      zs_deflate_plan e;
      plan(o, level, zs_make_params(15, 8), e);  // ... and the params entries at 15 / 8
      snprintf(name, sizeof name, "explicit/s%d/l%d", sweep, level);
      print_plan(name, e, kN);
      printf("case=route/default/s%d/l%d sweep=%d\n", sweep, level, p.sweep);
#endif
    }
#ifndef EMU_PLAN_BEFORE
  for (int wb = 8; wb <= 15; wb++)
    for (int ml = 1; ml <= 9; ml++) {
      const zs_deflate_params q = zs_make_params(wb, ml);
      zs_route_opts o;
      zs_deflate_plan p;
      plan(o, 6, q, p);
      const zs_fast_plan fg = zs_plan_fast_params(q, true, kN), fs = zs_plan_fast_params(q, false, kN);
      int fits = 1;  // every stream's blocks fit the records the plan gives it
      for (uint32_t i = 0; i < kN; i++) fits &= kLens[i] / q.sym_end + 1 <= (i + 1 < kN ? p.blk[i + 1] : p.B) - p.blk[i];
      printf("case=w%d/m%d default=%d w_bits=%u hash_bits=%u hash_shift=%u sym_end=%u sweep=%d nseg=%zu B=%u max_blk=%u "
             "codes=%zu hdr=%zu fits=%d group_route=%d group_lds=%u serial_route=%d serial_lds=%u ghead=%llu\n",
             wb, ml, q.is_default(), q.w_bits, q.hash_bits, q.hash_shift, q.sym_end, p.sweep, p.segs.size(), p.B, p.max_blk,
             p.codes_bytes, p.hdr_bytes, fits, (int)fg.route, fg.lds_bytes, (int)fs.route, fs.lds_bytes,
             (unsigned long long)fs.ghead_bytes);
    }
  const int bits[] = {-16, -15, -9, -8, -7, 0, 7, 8, 9, 15, 16, 23, 24, 25, 31, 32};
  for (int wbits : bits) {
    int wrap = -1;
    const int w = zs_wbits_split(wbits, &wrap);
    printf("case=wbits/%d window=%d wrap=%d\n", wbits, w, w ? wrap : -1);
  }
#endif
  return 0;
}
