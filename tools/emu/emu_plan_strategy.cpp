// emu_plan_strategy.cpp -- what csrc/zs_plan.h decides for a (level, strategy) pair
// (zs_plan_strategy) and zs_k_huff_tally's (stream, block) list (zs_plan_huff_chunks),
// printed one line of key=value pairs per case for tests/test_plan_strategy.py.  Plain
// C++, no ROCm headers.
//   g++ -std=c++17 -O2 -o emu_plan_strategy tools/emu/emu_plan_strategy.cpp && ./emu_plan_strategy
#include <stdio.h>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"

int main() {
  for (int rle_ref = 0; rle_ref <= 1; rle_ref++)
    for (int level = 0; level <= 9; level++)
      for (int strategy = 0; strategy <= 4; strategy++) {
        zs_route_opts o;
        o.rle_ref = rle_ref != 0;
        const zs_strategy_plan sp = zs_plan_strategy(o, level, strategy);
        // the workspace plan of three streams at the level the route asks for
        const uint32_t len[3] = {100, 70000, 0};
        zs_deflate_plan p;
        zs_deflate_req r;
        r.level = level;
        r.strategy = strategy;
        zs_plan_deflate(r, o, true, true, 3, len, nullptr, 0, p);
        printf("case=r%d/l%d/s%d stored=%d tally=%d filtered=%d fixed=%d wrap_strategy=%d plan_level=%d nwin=%zu pscr=%zu\n",
               rle_ref, level, strategy, sp.stored, sp.tally, sp.filtered, sp.fixed, sp.wrap_strategy, sp.plan_level,
               p.segs.size(), p.pscr_bytes);
      }
  const uint32_t lens[] = {0, 1, 16382, 16383, 16384, 32766, 200000};
  std::vector<zs_huff_chunk> ch;
  zs_plan_huff_chunks(7, lens, ch);
  printf("case=chunks n=%zu list=", ch.size());
  for (size_t i = 0; i < ch.size(); i++) printf("%s%u:%u", i ? "," : "", ch[i].s, ch[i].b);
  printf("\n");
  // every stream's blocks fit the records the workspace plan gives it
  zs_route_opts o;
  zs_deflate_plan p;
  zs_deflate_req r;
  r.level = 1;
  zs_plan_deflate(r, o, true, true, 7, lens, nullptr, 0, p);
  int fits = 1;
  for (uint32_t i = 0; i < 7; i++) fits &= lens[i] / ZS_SYM_END + 1 <= (i + 1 < 7 ? p.blk[i + 1] : p.B) - p.blk[i];
  printf("case=records fits=%d\n", fits);
  return 0;
}
