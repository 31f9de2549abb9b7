// emu_plan_launch -- what csrc/zs_plan.h decides about whole deflate calls, for
// tests/test_plan_launch.py.  Plain C++, no ROCm headers.
//   g++ -std=c++17 -O2 -Wall -Werror -o emu_plan_launch tools/emu/emu_plan_launch.cpp
//   ./emu_plan_launch           the launch trace each call of emu_launch_cases() implies: one line per
//                               kernel instance in launch order, with its grid, block and dynamic LDS
//   ./emu_plan_launch faults    the fault that wins in each call of emu_fault_cases()
//   ./emu_plan_launch layout    the metadata block's section offsets for a grid of batch shapes
//   ./emu_plan_launch combined  the verdict on dictionary requests with a strategy or parameters
// The steps around the pure functions are capi.cpp's: an entry makes its request, looks at the
// context, a host entry checks the whole batch and stages it, then deflate_device validates,
// finds the distinct dictionaries, plans and launches.
#include <stdio.h>
#include <string.h>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"
#include "../../zlib-streams-ts_amd/csrc/zs_dict.h"
#include "emu_plan_launch_cases.h"

static const char* const kErr[ZS_DE_COUNT] = {"ok",          "wbits",       "level",     "strategy",    "window_bits",
                                              "mem_level",   "dict_arrays", "dict_buffer", "dict_gzip", "dict_level0",
                                              "dict_long",   "params_level0", "rle_long", "align",      "dict_combined"};

static void line(const char* kernel, uint32_t gx, uint32_t gy, uint32_t block, uint32_t lds = 0) {
  printf("  %s grid=%u,%u block=%u lds=%u\n", kernel, gx, gy, block, lds);
}
static const char* name(const char* fmt, int a = 0, int b = 0, int c = 0) {
  static char buf[64];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  return buf;
}

// capi.cpp's deflate_launch, kernel by kernel
static void trace_launch(const zs_deflate_plan& p) {
  const uint32_t n = p.n, gs = p.g_streams;
  const int wrap = p.req.wrap;
  const bool par = p.variant == ZS_VAR_PAR;
  const char* sfx = par ? "_par" : p.variant == ZS_VAR_DICT ? "_dict" : p.variant == ZS_VAR_FILT ? "_filt" : "";
  const char* pw = p.pw == 4 ? "_4w" : p.pw == 2 ? "_2w" : "";
  if (p.stored) {
    if (wrap) line("zs_k_checksum", n, 1, 64);
    line("zs_k_stored", p.g_stored_x, n, 256);
    return;
  }
  if (wrap) {
    line("zs_k_checksum", n, 1, 64);
    line("zs_k_copy_check", gs, 1, 256);
  }
  if (p.match == ZS_MATCH_SWEEP) {
    line(name("zs_k_bucket<%d>", p.lane_order), (uint32_t)p.segs.size(), 1, 512);
    line(name("zs_k_sweep<%d>", p.sweep_u8), (uint32_t)p.segs.size(), 1, 1024);
  } else if (p.match == ZS_MATCH_CHAIN) {
    line(name(par ? "zs_k_prev_par<%d>" : "zs_k_prev<%d>", p.lane_order), n, 1, 64);
    if (p.max_len) line(par ? "zs_k_match_par" : "zs_k_match", p.g_match_x, n, 1024);
  }
  switch (p.sym) {
    case ZS_SYM_HUFF: line("zs_k_huff_tally", (uint32_t)p.chunks.size(), 1, 256); break;
    case ZS_SYM_RLE: line("zs_k_rle_tally", n, 1, 256); break;
    case ZS_SYM_PARSE: {
      char k[64];
      snprintf(k, sizeof k, "zs_k_parse%s%s", pw, sfx);
      line(k, n, 1, 64u * p.pw);
      break;
    }
    case ZS_SYM_FAST_GROUP:
      line(name(par ? "zs_k_fast_par<%d,%d,%d>" : "zs_k_fast<%d,%d,%d>", p.nice_bucket, p.lane_order, p.dict), n, 1, 64,
           p.fast_lds);
      break;
    default:
      if (par) line(name("zs_k_fast_serial_par<0,%d>", p.sym == ZS_SYM_FAST_SERIAL_GHEAD), n, 1, 64, p.fast_lds);
      else line(name("zs_k_fast_serial<%d>", p.dict), n, 1, 64, p.fast_lds);
  }
  line(par ? "zs_k_trees_par" : "zs_k_trees", p.max_blk, n, 64);
  line(p.dict ? "zs_k_layout_dict" : "zs_k_layout", gs, 1, 256);
  line("zs_k_emit", p.max_blk, n, 256);
  if (wrap) line(p.dict ? "zs_k_wrap_dict" : par ? "zs_k_wrap_par" : "zs_k_wrap", gs, 1, 256);
  line("zs_k_finish", gs, 1, 256);
}

// An entry's request (before the context is looked at)
static zs_deflate_err make_req(const emu_call& k, zs_deflate_req* r) {
  if (k.family == EMU_PARAMS) return zs_deflate_make_req_params(k.level, k.wbits, k.mem_level, r);
  return zs_deflate_make_req(k.level, k.wbits, k.family == EMU_STRATEGY ? k.strategy : ZS_STRAT_DEFAULT,
                             k.family == EMU_DICT, r);
}

// The call from its entry to the launch: prints the trace (trace set) and returns the fault
// that ends it, or "ok"; "null_context" is the entries' own check.
static const char* run(const emu_call& k, bool trace) {
  zs_route_opts o;
  o.match_sweep = k.match_sweep != 0;
  o.rle_ref = k.rle_ref != 0;
  zs_deflate_req req;
  if (const zs_deflate_err e = make_req(k, &req)) return kErr[e];
  if (k.null_ctx) return "null_context";
  static const uint64_t z64 = 0;
  static const uint32_t z32 = 0;
  zs_deflate_call a;
  a.n = (uint32_t)k.in_len.size();
  a.in_len = k.in_len.data();
  a.dict_arrays = k.family == EMU_DICT && k.dict_null != EMU_DICT_NULL_ARRAYS;
  a.dict_buf = k.family == EMU_DICT && k.dict_null != EMU_DICT_NULL_BUFFER;
  const uint64_t* dict_off = !a.dict_arrays ? nullptr : k.dict_off.empty() ? &z64 : k.dict_off.data();
  a.dict_len = !a.dict_arrays ? nullptr : k.dict_len.empty() ? &z32 : k.dict_len.data();
  std::vector<uint64_t> out_off(k.out_off.begin(), k.out_off.end());
  if (k.host) {
    if (const zs_deflate_err e = zs_deflate_validate_host(req, a)) return kErr[e];
    if (a.n == 0) return "ok";
    req.dict = zs_deflate_any_dict(req, a);  // (a batch without any dictionary is the plain batch)
    if (!req.dict) a.dict_arrays = a.dict_buf = false, a.dict_len = nullptr;
    else a.dict_buf = true;                                // (the staged dictionaries)
    for (size_t i = 0; i < out_off.size(); i++)            // (the staged regions: capacities rounded up to words)
      out_off[i] = i ? out_off[i - 1] + ((k.out_cap[i - 1] + 3ull) & ~3ull) : 0;
  }
  a.out_off = out_off.data();
  a.out_cap = k.out_cap.data();
  a.caller_regions = !k.host;
  if (const zs_deflate_err e = zs_deflate_validate(req, o, a)) return kErr[e];
  if (a.n == 0) return "ok";
  zs_dict_set ds;
  if (req.dict) zs_dict_distinct(a.n, dict_off, a.dict_len, ds);
  zs_deflate_plan p;
  zs_plan_deflate(req, o, k.fast_group != 0, k.lane_order != 0, a.n, a.in_len, ds.any ? a.dict_len : nullptr,
                  (uint32_t)ds.uoff.size(), p);
  if (!trace) return "ok";
  if (p.dict) {  // the dictionary pre-step: DICTID of the distinct dictionaries (zlib), the joined streams
    if (req.wrap == 1) line("zs_k_checksum", p.ndict, 1, 64);
    line("zs_k_dict_join", p.g_join_x, a.n, 256);
  }
  trace_launch(p);
  line("zs_k_deflate_check", (a.n + 255) / 256, 1, 256);  // (with the caller's check array given)
  return "ok";
}

static void layouts() {
  for (uint32_t n : {1u, 3u, 257u})
    for (uint32_t ndict : {0u, 1u, 2u})
      for (size_t nchunks : {(size_t)0, (size_t)n + 12})
        for (uint32_t nwin : {0u, n + 6}) {
          const zs_meta_layout m(n, nwin, ndict != 0, ndict, nchunks);
          printf("case=n%u/dict%u/chunks%zu/win%u n=%u ndict=%u nchunks=%zu nwin=%u in_off=%zu in_len=%zu out_off=%zu "
                 "out_cap=%zu pos_base=%zu blk_base=%zu segs=%zu doff=%zu dlen=%zu did=%zu start=%zu joff=%zu jlen=%zu "
                 "uoff=%zu ulen=%zu chunks=%zu bytes=%zu\n",
                 n, ndict, nchunks, nwin, n, ndict, nchunks, nwin, m.in_off, m.in_len, m.out_off, m.out_cap, m.pos_base,
                 m.blk_base, m.segs, m.doff, m.dlen, m.did, m.start, m.joff, m.jlen, m.uoff, m.ulen, m.chunks, m.bytes);
        }
  // ... and as zs_plan_deflate fills it: sweep windows, dictionaries (two distinct), Huffman chunks
  const uint32_t lens[3] = {100, 70000, 0}, dl[3] = {300, 300, 5};
  zs_route_opts o;
  zs_deflate_plan p;
  zs_deflate_req r;
  r.dict = true;
  zs_plan_deflate(r, o, true, true, 3, lens, dl, 2, p);
  printf("case=plan/dict dict=%d ndict=%u nwin=%zu nchunks=%zu bytes=%zu chunks=%zu ulen=%zu\n", p.dict, p.ndict,
         p.segs.size(), p.chunks.size(), p.ml.bytes, p.ml.chunks, p.ml.ulen);
  r.dict = false;
  r.strategy = ZS_STRAT_HUFFMAN_ONLY;
  zs_plan_deflate(r, o, true, true, 3, lens, nullptr, 0, p);
  printf("case=plan/huff dict=%d ndict=%u nwin=%zu nchunks=%zu bytes=%zu chunks=%zu ulen=%zu\n", p.dict, p.ndict,
         p.segs.size(), p.chunks.size(), p.ml.bytes, p.ml.chunks, p.ml.ulen);
}

// Requests no entry makes: dictionaries with a strategy, or with parameters
static void combined() {
  const uint32_t len[2] = {100, 5}, cap[2] = {1024, 1024}, dl[2] = {0, 300};
  const uint64_t off[2] = {0, 1024};
  zs_deflate_call a;
  a.n = 2;
  a.in_len = len;
  a.out_off = off;
  a.out_cap = cap;
  a.dict_arrays = a.dict_buf = true;
  a.dict_len = dl;
  zs_deflate_req r;
  zs_deflate_make_req(6, 15, ZS_STRAT_FILTERED, true, &r);
  printf("strategy=%s\n", kErr[zs_deflate_validate(r, zs_route_opts(), a)]);
  zs_deflate_make_req(6, 15, ZS_STRAT_DEFAULT, true, &r);
  r.q = zs_make_params(12, 8);
  printf("params=%s\n", kErr[zs_deflate_validate(r, zs_route_opts(), a)]);
  r.q = zs_deflate_params();
  printf("plain=%s\n", kErr[zs_deflate_validate(r, zs_route_opts(), a)]);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "layout")) {
    layouts();
  } else if (argc > 1 && !strcmp(argv[1], "combined")) {
    combined();
  } else if (argc > 1 && !strcmp(argv[1], "faults")) {
    for (const emu_call& k : emu_fault_cases()) printf("case=%s fault=%s\n", k.name.c_str(), run(k, false));
  } else {
    for (const emu_call& k : emu_launch_cases()) {
      printf("case=%s\n", k.name.c_str());
      const char* e = run(k, true);
      if (strcmp(e, "ok")) printf("  fault=%s\n", e);
    }
  }
  return 0;
}
