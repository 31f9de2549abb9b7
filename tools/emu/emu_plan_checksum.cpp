// emu_plan_checksum.cpp -- what csrc/zs_plan.h decides about a batch's data checksum
// (zs_plan_checksum: one wave per stream, or parts of checksum_part bytes once a stream's length
// bound passes checksum_split), the values zs_set_option takes for the two options, and the
// deflate plan beside it, which the options must leave alone; printed one line of key=value
// pairs per case for tests/test_plan_checksum.py.  Plain C++, no ROCm headers.
//   g++ -std=c++17 -O2 -o emu_plan_checksum tools/emu/emu_plan_checksum.cpp && ./emu_plan_checksum
// (also as a stand-alone program with -fsanitize=address,undefined)
#include <stdio.h>

#include <string>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"

static const uint32_t kLens[] = {0, 1, 100, 16383, 65537, 65538, 200000};
static const uint32_t kN = 7;

// as emu_plan_params.cpp prints a plan: the figures tests/test_plan_params.py pins as BEFORE
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

static std::string list(const std::vector<uint32_t>& v) {
  std::string s;
  for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
  return s.empty() ? "-" : s;
}

// the plan of one batch of length bounds; the map is printed only when it is short
static void plan(const char* name, const zs_route_opts& o, const std::vector<uint32_t>& bound) {
  zs_checksum_plan p;
  p.split = true;  // (a plan object is reused across calls: whatever it held must go)
  p.P = 77;
  p.pfirst.assign(3, 9);
  p.pstream.assign(5, 9);
  zs_plan_checksum(o, (uint32_t)bound.size(), bound.data(), p);
  // every part's stream is the one whose range holds it
  int ok = 1;
  for (uint32_t i = 0; p.split && i < bound.size(); i++)
    for (uint32_t k = p.pfirst[i]; k < p.pfirst[i + 1]; k++) ok &= p.pstream[k] == i;
  printf("case=%s split=%d part_lg=%u parts=%u ws=%zu map=%zu pstream_at=%zu npfirst=%zu npstream=%zu ok=%d", name,
         (int)p.split, p.part_lg, p.P, p.ws_bytes, p.map_bytes(), p.split ? p.map_pstream() : 0, p.pfirst.size(),
         p.pstream.size(), ok);
  if (p.P <= 64) printf(" pfirst=%s pstream=%s", list(p.pfirst).c_str(), list(p.pstream).c_str());
  printf("\n");
}

int main() {
  char name[64];
  // the deflate plan with the two options at their defaults and at the tests' small values
  for (int small = 0; small <= 1; small++)
    for (int sweep = 0; sweep <= 1; sweep++)
      for (int level : {1, 6}) {
        zs_route_opts o;
        o.match_sweep = sweep != 0;
        if (small) {
          o.checksum_split = 1;
          o.checksum_part = 1024;
        }
        zs_deflate_req r;
        zs_deflate_make_req(level, 31, ZS_STRAT_DEFAULT, false, &r);
        zs_deflate_plan p;
        zs_plan_deflate(r, o, true, true, kN, kLens, nullptr, 0, p);
        snprintf(name, sizeof name, "%s/s%d/l%d", small ? "small" : "default", sweep, level);
        print_plan(name, p, kN);
      }
  {
    const zs_route_opts o;
    printf("case=defaults split=%u part=%u\n", o.checksum_split, o.checksum_part);
    // the benchmark's and the golden tests' streams: at most 256 KiB
    plan("default/256k", o, std::vector<uint32_t>(4096, 262144));
    plan("default/at_split", o, {100, 1u << 18, 0});
    plan("default/past_split", o, {100, (1u << 18) + 1, 0});
    plan("default/4g", o, {0xffffffffu});
    plan("default/empty_batch", o, {});
  }
  {
    zs_route_opts o;
    o.checksum_split = 4096;
    o.checksum_part = 1024;
    plan("p1024/below", o, {0, 1, 4095, 4096});
    plan("p1024/map", o, {0, 1, 1024, 1025, 3072, 4097});
    o.checksum_split = 1024;
    plan("p1024/issue", o, {0, 1, 1024, 1025, 3072});
    o.checksum_split = 0;
    plan("p1024/never", o, {0, 1, 1024, 1025, 3072, 0xffffffffu});
    // more parts than one launch takes: one wave per stream
    o.checksum_split = 1;
    plan("p1024/too_many", o, std::vector<uint32_t>(5, 0xffffffffu));
    plan("p1024/most", o, std::vector<uint32_t>(4, 0xffffffffu));
    o.checksum_part = 1u << 20;
    plan("p1m/4g", o, {0xffffffffu, 2});
  }
  for (int v : {-1, 0, 1, 4096, 1 << 20, 0x7fffffff}) printf("case=opt/split/%d ok=%d\n", v, (int)zs_checksum_split_ok(v));
  for (int v : {-1024, -1, 0, 1, 512, 1023, 1024, 1025, 3072, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 21, 0x40000000})
    printf("case=opt/part/%d ok=%d\n", v, (int)zs_checksum_part_ok(v));
  return 0;
}
