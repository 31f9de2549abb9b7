// emu_rle.cpp -- host build of csrc/zs_rle.h, the closed form of zlib's deflate_rle that
// zs_k_rle_tally (deflate_strategy.hip) evaluates per position.  Reads a file, prints
// the symbols the closed form gives for it, one hex word per line ("s <word>"), and the
// block records cut after every 16,383rd symbol ("b <sym_start> <sym_count> <in_start>
// <in_end> <last>"), as the kernel writes them.  The symbols are computed twice -- per
// position (zs_rle_at, from each position's run start and an end looked for at most 258
// bytes ahead, as the kernel does) and per run (zs_rle_run_syms / zs_rle_run_sym_at) --
// and the program fails when the two differ.  tests/test_rle_model.py compares the
// output with a sequential restatement of deflate_rle and with zlib itself.
//   g++ -std=c++17 -O2 -o emu_rle tools/emu/emu_rle.cpp && ./emu_rle input.bin
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../zlib-streams-ts_amd/csrc/zs_common.h"
#include "../../zlib-streams-ts_amd/csrc/zs_rle.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> in;
  for (int ch; (ch = fgetc(f)) != EOF;) in.push_back((uint8_t)ch);
  fclose(f);
  const uint32_t n = (uint32_t)in.size();
  // per position
  std::vector<uint32_t> sym, at;
  for (uint32_t p = 0, s = 0; p < n; p++) {
    if (p > 0 && in[p] != in[p - 1]) s = p;
    uint64_t e = (uint64_t)p + 2 * ZS_RLE_MAX;  // "beyond": no run start within 258 bytes
    for (uint32_t q = p + 1; q <= p + ZS_RLE_MAX; q++)
      if (q >= n || in[q] != in[q - 1]) {
        e = q;
        break;
      }
    const uint32_t v = zs_rle_at(p, s, e, in[p]);
    if (v != ZS_RLE_NONE) {
      sym.push_back(v);
      at.push_back(p);
    }
  }
  // per run
  size_t k = 0;
  for (uint32_t s = 0; s < n;) {
    uint32_t e = s + 1;
    while (e < n && in[e] == in[s]) e++;
    const uint32_t cnt = zs_rle_run_syms(e - s);
    for (uint32_t j = 0; j < cnt; j++, k++) {
      uint32_t len;
      const uint64_t off = zs_rle_run_sym_at(e - s, j, &len);
      const uint32_t want = len == 1 ? in[s] : zs_rle_match(len);
      if (k >= sym.size() || sym[k] != want || at[k] != s + off) {
        fprintf(stderr, "symbol %zu of the run at %u differs between the two forms\n", k, s);
        return 1;
      }
    }
    s = e;
  }
  if (k != sym.size()) return 1;
  for (uint32_t v : sym) printf("s %08x\n", v);
  const uint32_t total = (uint32_t)sym.size(), nflush = total / ZS_SYM_END;
  for (uint32_t b = 0; b <= nflush; b++) {
    auto end_of = [&](uint32_t g) { return at[g] + ((sym[g] & 0x80000000u) ? ((sym[g] >> 16) & 0xffu) + ZS_MIN_MATCH : 1u); };
    const uint32_t in_start = b == 0 ? 0u : end_of(b * ZS_SYM_END - 1), in_end = b < nflush ? end_of((b + 1) * ZS_SYM_END - 1) : n;
    printf("b %u %u %u %u %u\n", b * ZS_SYM_END, b < nflush ? (uint32_t)ZS_SYM_END : total - nflush * ZS_SYM_END, in_start,
           in_end, b == nflush ? 1u : 0u);
  }
  return 0;
}
