// emu_plan_launch_cases.h -- the batches tools/emu/emu_plan_launch.cpp prints the launch trace,
// the metadata layout and the validation verdict of.  Inputs only: calls as the C entries
// receive them, so that whatever walks the list (the emulator; the instrumented copy of the
// host layer the expected tables were recorded from) sees the same ones in the same order.
#ifndef EMU_PLAN_LAUNCH_CASES_H
#define EMU_PLAN_LAUNCH_CASES_H
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

enum { EMU_PLAIN = 0, EMU_STRATEGY, EMU_PARAMS, EMU_DICT };  // the four families of zs_deflate_batch* entries
enum { EMU_DICT_NULL_ARRAYS = 1, EMU_DICT_NULL_BUFFER = 2 };

struct emu_call {
  std::string name;
  int family = EMU_PLAIN;
  bool host = false;      // the host entry of the family (else the _device one)
  bool null_ctx = false;
  int level = 6, wbits = 15, strategy = 0, mem_level = 8;
  // options (zs_set_option)
  int match_sweep = 1, fast_group = 1, lane_order = 1, rle_ref = 1;
  std::vector<uint32_t> in_len, out_off, out_cap, dict_len;  // (dict_len: EMU_DICT)
  std::vector<uint64_t> dict_off;
  int dict_null = 0;      // EMU_DICT_NULL_*
};

static const uint32_t kEmuLens[7] = {0, 1, 100, 16383, 65537, 65538, 200000};

// n streams of the lengths above in turn, capacities and offsets multiples of 4
static inline emu_call emu_batch(const std::string& name, int family, int level, int wbits, uint32_t n = 7) {
  emu_call c;
  c.name = name;
  c.family = family;
  c.level = level;
  c.wbits = wbits;
  uint32_t off = 0;
  for (uint32_t i = 0; i < n; i++) {
    c.in_len.push_back(kEmuLens[i % 7]);
    c.out_cap.push_back((kEmuLens[i % 7] + 1024) & ~3u);
    c.out_off.push_back(off);
    off += c.out_cap.back();
  }
  return c;
}
// dictionaries of `lens` in turn: the second and third stream share one, the others have their own
static inline void emu_dicts(emu_call& c, const std::vector<uint32_t>& lens) {
  uint64_t off = 0;
  for (size_t i = 0; i < c.in_len.size(); i++) {
    c.dict_len.push_back(lens[i % lens.size()]);
    if (i == 2 && c.dict_len[1] == c.dict_len[2]) off = c.dict_off[1];
    c.dict_off.push_back(off);
    off += c.dict_len.back();
  }
}
static inline std::string emu_fmt(const char* fmt, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0,
                                  int f = 0) {
  char buf[128];
  snprintf(buf, sizeof buf, fmt, a, b, c, d, e, f);
  return buf;
}

// Every route of the launch: levels 0..9, the wrappers, the strategies, the parameter pairs,
// dictionaries (and dictionary entries without any), the options, n around ZS_PARSE2W_AUTO.
static inline std::vector<emu_call> emu_launch_cases() {
  std::vector<emu_call> v;
  const int wb[3] = {-15, 15, 31};
  for (int level = 0; level <= 9; level++)
    for (int w = 0; w < 3; w++) v.push_back(emu_batch(emu_fmt("plain/l%d/w%d", level, w), EMU_PLAIN, level, wb[w]));
  for (int level = 1; level <= 9; level++)
    for (int opts = 0; opts < 8; opts++) {
      emu_call c = emu_batch(emu_fmt("opts/l%d/sweep%d/group%d/order%d", level, opts & 1, opts >> 1 & 1, opts >> 2), EMU_PLAIN,
                             level, 15);
      c.match_sweep = opts & 1;
      c.fast_group = opts >> 1 & 1;
      c.lane_order = opts >> 2;
      v.push_back(c);
    }
  for (int level : {3, 6})
    for (uint32_t n : {2047u, 2048u}) v.push_back(emu_batch(emu_fmt("n%d/l%d", (int)n, level), EMU_PLAIN, level, -15, n));
  for (int strategy = 1; strategy <= 4; strategy++)
    for (int rle_ref = 0; rle_ref <= 1; rle_ref++)
      for (int level : {0, 1, 3, 4, 6, 9})
        for (int w : {0, 2}) {
          emu_call c = emu_batch(emu_fmt("strategy%d/ref%d/l%d/w%d", strategy, rle_ref, level, w), EMU_STRATEGY, level, wb[w]);
          c.strategy = strategy;
          c.rle_ref = rle_ref;
          v.push_back(c);
        }
  const int pairs[6][2] = {{9, 1}, {15, 9}, {14, 9}, {13, 9}, {12, 8}, {15, 8}};
  for (const auto& pr : pairs)
    for (int level : {1, 2, 3, 4, 6, 9})
      for (int opts = 0; opts < 4; opts++)
        for (int w : {0, 1}) {
          if (w == 0 && level != 1 && level != 6) continue;
          emu_call c = emu_batch(emu_fmt("params%d_%d/l%d/group%d_order%d/w%d", pr[0], pr[1], level, opts & 1, opts >> 1, w),
                                 EMU_PARAMS, level, w == 0 ? -pr[0] : pr[0]);
          c.mem_level = pr[1];
          c.fast_group = opts & 1;
          c.lane_order = opts >> 1;
          v.push_back(c);
        }
  for (int level = 1; level <= 9; level++)
    for (int w : {0, 1})
      for (int zero = 0; zero <= 1; zero++)
        for (int opts = 0; opts < 8; opts++) {
          if (opts != 7 && level != 1 && level != 6) continue;  // (the options at a level of each kind)
          emu_call c = emu_batch(emu_fmt("dict%d/l%d/w%d/opts%d", zero ? 0 : 1, level, w, opts), EMU_DICT, level, wb[w]);
          emu_dicts(c, zero ? std::vector<uint32_t>{0} : std::vector<uint32_t>{300, 40000, 40000, 0, 32768});
          c.match_sweep = opts & 1;
          c.fast_group = opts >> 1 & 1;
          c.lane_order = opts >> 2;
          v.push_back(c);
        }
  return v;
}

// Faulty calls, some with several faults at once, of every entry family
static inline std::vector<emu_call> emu_fault_cases() {
  std::vector<emu_call> v;
  auto add = [&](emu_call c, bool host) {
    c.host = host;
    c.name += host ? "/host" : "/device";
    v.push_back(c);
  };
  for (int host = 0; host <= 1; host++) {
    emu_call c = emu_batch("ok", EMU_PLAIN, 6, 15);
    add(c, host);
    c = emu_batch("default_level", EMU_PLAIN, -1, 15);
    add(c, host);
    c = emu_batch("wbits", EMU_PLAIN, 6, 14);
    add(c, host);
    c = emu_batch("wbits+level", EMU_PLAIN, 10, 47);
    add(c, host);
    c = emu_batch("level", EMU_PLAIN, -2, 31);
    add(c, host);
    c = emu_batch("level+null_ctx", EMU_PLAIN, 11, 15);
    c.null_ctx = true;
    add(c, host);
    c = emu_batch("level+align", EMU_PLAIN, 10, 15);
    c.out_off[1] += 2;
    add(c, host);
    c = emu_batch("align_off", EMU_PLAIN, 6, 15);
    c.out_off[1] += 2;
    add(c, host);
    c = emu_batch("align_cap", EMU_PLAIN, 6, 15);
    c.out_cap[2] += 1;
    add(c, host);
    c = emu_batch("empty+level", EMU_PLAIN, 12, 15, 0);
    add(c, host);
    c = emu_batch("empty+wbits", EMU_PLAIN, 6, 0, 0);
    add(c, host);
    c = emu_batch("empty", EMU_PLAIN, 6, 15, 0);
    add(c, host);

    c = emu_batch("strategy", EMU_STRATEGY, 6, 15);
    c.strategy = 5;
    add(c, host);
    c = emu_batch("strategy+null_ctx", EMU_STRATEGY, 6, 15);
    c.strategy = -1;
    c.null_ctx = true;
    add(c, host);
    c = emu_batch("strategy+wbits+level", EMU_STRATEGY, 10, 16);
    c.strategy = 5;
    add(c, host);
    c = emu_batch("strategy_ok+level", EMU_STRATEGY, 10, 15);
    c.strategy = 3;
    add(c, host);
    c = emu_batch("empty+strategy", EMU_STRATEGY, 6, 15, 0);
    c.strategy = 7;
    add(c, host);
    c = emu_batch("rle_long", EMU_STRATEGY, 6, 15);
    c.strategy = 3;
    c.rle_ref = 0;
    c.in_len[3] = 0xffff0001u;
    add(c, host);
    c = emu_batch("rle_long_ref", EMU_STRATEGY, 6, 15);  // (the reference's Z_RLE is the Huffman tally: no limit)
    c.strategy = 3;
    c.in_len[3] = 0xffff0001u;
    add(c, host);
    c = emu_batch("rle_long+align", EMU_STRATEGY, 6, 15);
    c.strategy = 3;
    c.rle_ref = 0;
    c.in_len[3] = 0xffff0001u;
    c.out_off[0] = 1;
    add(c, host);
    c = emu_batch("rle_long_level0", EMU_STRATEGY, 0, 15);
    c.strategy = 3;
    c.rle_ref = 0;
    c.in_len[3] = 0xffff0001u;
    add(c, host);

    c = emu_batch("window_bits", EMU_PARAMS, 6, 7);
    add(c, host);
    c = emu_batch("window_bits_raw8", EMU_PARAMS, 6, -8);
    add(c, host);
    c = emu_batch("window_bits+mem_level+null_ctx", EMU_PARAMS, 6, 32);
    c.mem_level = 0;
    c.null_ctx = true;
    add(c, host);
    c = emu_batch("mem_level+null_ctx", EMU_PARAMS, 6, 12);
    c.mem_level = 10;
    c.null_ctx = true;
    add(c, host);
    c = emu_batch("mem_level+level", EMU_PARAMS, 10, 12);
    c.mem_level = 0;
    add(c, host);
    c = emu_batch("params_ok+level", EMU_PARAMS, 10, 12);
    add(c, host);
    c = emu_batch("params_level0", EMU_PARAMS, 0, 12);
    add(c, host);
    c = emu_batch("params_level0+align", EMU_PARAMS, 0, 12);
    c.out_off[3] = 2;
    add(c, host);
    c = emu_batch("params_default_level0", EMU_PARAMS, 0, 15);
    add(c, host);
    c = emu_batch("empty+params_level0", EMU_PARAMS, 0, 12, 0);
    add(c, host);
    c = emu_batch("empty+mem_level", EMU_PARAMS, 6, 12, 0);
    c.mem_level = 10;
    add(c, host);

    const std::vector<uint32_t> some = {300, 0, 40000}, none = {0};
    c = emu_batch("dict_ok", EMU_DICT, 6, 15);
    emu_dicts(c, some);
    add(c, host);
    c = emu_batch("dict_null_ctx+arrays", EMU_DICT, 6, 15);
    emu_dicts(c, some);
    c.null_ctx = true;
    c.dict_null = EMU_DICT_NULL_ARRAYS;
    add(c, host);
    c = emu_batch("dict_arrays+level", EMU_DICT, 10, 15);
    emu_dicts(c, some);
    c.dict_null = EMU_DICT_NULL_ARRAYS;
    add(c, host);
    c = emu_batch("dict_arrays+wbits", EMU_DICT, 6, 3);
    emu_dicts(c, some);
    c.dict_null = EMU_DICT_NULL_ARRAYS;
    add(c, host);
    c = emu_batch("empty+dict_arrays", EMU_DICT, 6, 15, 0);
    c.dict_null = EMU_DICT_NULL_ARRAYS;
    add(c, host);
    c = emu_batch("empty+dict_buffer+level", EMU_DICT, 10, 15, 0);
    c.dict_null = EMU_DICT_NULL_BUFFER;
    add(c, host);
    c = emu_batch("dict_buffer", EMU_DICT, 6, 15);
    emu_dicts(c, some);
    c.dict_null = EMU_DICT_NULL_BUFFER;
    add(c, host);
    c = emu_batch("dict_buffer_unused", EMU_DICT, 6, 15);  // (no stream has a dictionary: the plain batch)
    emu_dicts(c, none);
    c.dict_null = EMU_DICT_NULL_BUFFER;
    add(c, host);
    c = emu_batch("dict_buffer+gzip+level0", EMU_DICT, 0, 31);
    emu_dicts(c, some);
    c.dict_null = EMU_DICT_NULL_BUFFER;
    add(c, host);
    c = emu_batch("dict_gzip", EMU_DICT, 6, 31);
    emu_dicts(c, some);
    add(c, host);
    c = emu_batch("dict_none_gzip_level0", EMU_DICT, 0, 31);
    emu_dicts(c, none);
    add(c, host);
    c = emu_batch("dict_gzip+level0+align", EMU_DICT, 0, 31);
    emu_dicts(c, some);
    c.out_off[0] = 2;
    add(c, host);
    c = emu_batch("dict_level0", EMU_DICT, 0, 15);
    emu_dicts(c, some);
    add(c, host);
    c = emu_batch("dict_level0+wbits", EMU_DICT, 0, 7);
    emu_dicts(c, some);
    add(c, host);
    c = emu_batch("dict_gzip+level", EMU_DICT, 10, 31);
    emu_dicts(c, some);
    add(c, host);
    c = emu_batch("dict_level", EMU_DICT, 10, 15);
    emu_dicts(c, some);
    add(c, host);
    c = emu_batch("dict_long", EMU_DICT, 6, 15);
    emu_dicts(c, some);
    c.in_len[2] = 0xffff8000u;
    add(c, host);
    c = emu_batch("dict_long_without", EMU_DICT, 6, 15);  // (the long stream has no dictionary)
    emu_dicts(c, some);
    c.in_len[1] = 0xffff8000u;
    add(c, host);
    c = emu_batch("dict_long+align", EMU_DICT, 6, 15);
    emu_dicts(c, some);
    c.in_len[2] = 0xffff8000u;
    c.out_off[4] = 2;
    add(c, host);
    c = emu_batch("dict_align_cap", EMU_DICT, 6, -15);
    emu_dicts(c, some);
    c.out_cap[0] += 2;
    add(c, host);
  }
  return v;
}

#endif
