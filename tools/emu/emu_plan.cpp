// emu_plan -- prints what csrc/zs_plan.h decides for a fixed set of batches, one
// line of key=value pairs per case (tests/test_plan_model.py holds the expected
// values).  Host only: g++ -std=c++17 -O2 -Wall -Werror, no ROCm headers.
#include <stdio.h>

#include <string>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"

// a list of indices as ranges: "0-6,9" ("-" when empty)
static std::string ranges(const std::vector<uint32_t>& v) {
  std::string s;
  for (size_t i = 0; i < v.size();) {
    size_t j = i;
    while (j + 1 < v.size() && v[j + 1] == v[j] + 1) j++;
    if (!s.empty()) s += ",";
    s += std::to_string(v[i]);
    if (j > i) s += "-" + std::to_string(v[j]);
    i = j + 1;
  }
  return s.empty() ? "-" : s;
}

struct Member {
  uint32_t in_len, out_cap;
};

// the inflate plan of a batch, and the segmented plan of its segmented members
static void inflate_case(const char* name, const zs_route_opts& o, int wbits, const std::vector<Member>& m) {
  std::vector<uint32_t> in_len, out_cap;
  for (const Member& x : m) {
    in_len.push_back(x.in_len);
    out_cap.push_back(x.out_cap);
  }
  zs_inflate_plan p;
  zs_plan_inflate(o, wbits, (uint32_t)m.size(), in_len.data(), out_cap.data(), p);
  printf("case=%s n=%zu seg=%s split=%s wave=%s wave_min=%u lane_block=%u lane_rt=%d piece_cap=%u val_stride=%llu "
         "wave_refw=%d wave_lanes=%d wave_block=%u wave_rt=%d",
         name, m.size(), ranges(p.seg).c_str(), ranges(p.split).c_str(), ranges(p.wave).c_str(), p.wave_min,
         p.lane.block, p.lane.rt, p.piece_cap, (unsigned long long)p.val_stride, (int)p.wave_refw, (int)p.wave_lanes,
         p.wave_lane.block, p.wave_lane.rt);
  if (!p.seg.empty()) {
    zs_seg_plan g;
    zs_plan_seg(o, wbits, p.seg, in_len.data(), out_cap.data(), g);
    const size_t ng = p.seg.size();
    // (slots0, pmax0, scr0: the first segmented member's share of the prefix arrays)
    printf(" walk=%d/%u/%d bits=%u seg_split=%d big=%s nwalk=%u resolve=%s decode=%d/%d slots0=%u pmax0=%u scr0=%llu "
           "slots=%u pieces=%u scr=%llu gdec=%u gfb=%u",
           (int)g.d64, g.w2k ? 2048u : 1024u, (int)(g.large && !g.d64), g.walk_bits, g.split, ranges(g.big).c_str(),
           g.nwalk, g.rsmall ? "512/65536" : "256/32768", (int)g.d64, (int)g.refw, g.spb[1], g.pbase[1],
           (unsigned long long)g.sbase[1], g.nb, g.pbase[ng], (unsigned long long)g.sbase[ng], g.gdec, g.gfb);
  }
  printf("\n");
}

static void deflate_case(const char* name, const zs_route_opts& o, int level, const std::vector<uint32_t>& in_len) {
  zs_deflate_plan p;
  zs_deflate_req r;
  r.level = level;
  zs_plan_deflate(r, o, true, true, (uint32_t)in_len.size(), in_len.data(), nullptr, 0, p);
  printf("case=%s n=%zu P=%llu B=%u members=%llu max_len=%u max_blk=%u pw=%d nwin=%zu pos=", name, in_len.size(),
         (unsigned long long)p.P, p.B, (unsigned long long)p.members, p.max_len, p.max_blk, p.pw, p.segs.size());
  for (size_t i = 0; i < p.pos.size() && i < 4; i++) printf("%s%llu", i ? "," : "", (unsigned long long)p.pos[i]);
  printf(" blk=");
  for (size_t i = 0; i < p.blk.size() && i < 4; i++) printf("%s%u", i ? "," : "", p.blk[i]);
  printf(" win0=");
  for (size_t i = 0; i < p.win0.size() && i < 5; i++) printf("%s%u", i ? "," : "", p.win0[i]);
  printf(" wins=");  // stream:base:olo:ohi:mb of the first windows
  for (size_t i = 0; i < p.segs.size() && i < 4; i++)
    printf("%s%u:%u:%u:%u:%llu", i ? "," : "", p.segs[i].s, p.segs[i].base, p.segs[i].olo, p.segs[i].ohi,
           (unsigned long long)p.segs[i].mb);
  printf(" prevd=%zu mres=%zu syms=%zu pscr=%zu codes=%zu hdr=%zu\n", p.prevd_bytes, p.mres_bytes, p.syms_bytes,
         p.pscr_bytes, p.codes_bytes, p.hdr_bytes);
}

int main() {
  const zs_route_opts def;  // every option at its default (256 compute units)
  const Member tiny{100, 1024};
  for (uint32_t n : {512u, 4608u, 4609u, 8192u, 16384u, 16385u, 32768u, 65536u})
    inflate_case(("lane" + std::to_string(n)).c_str(), def, -15, std::vector<Member>(n, tiny));
  {
    zs_route_opts o;
    o.lane_block = 8;
    for (uint32_t n : {512u, 65536u})
      inflate_case(("lane8_" + std::to_string(n)).c_str(), o, -15, std::vector<Member>(n, tiny));
    o.lane_block = 32;
    inflate_case("lane32_512", o, -15, std::vector<Member>(512, tiny));
  }
  inflate_case("P1", def, -15, std::vector<Member>(65536, {20000, 65536}));
  inflate_case("P2", def, 31, std::vector<Member>(8192, {20000, 65536}));
  inflate_case("P3", def, -15, std::vector<Member>(512, {90000, 262144}));
  inflate_case("P3_1024", def, -15, std::vector<Member>(1024, {90000, 262144}));
  inflate_case("P4", def, -15, std::vector<Member>(16, {1000, 1048576}));
  {
    zs_route_opts o;
    o.inflate_ref_wrap = false;
    inflate_case("P4_nowrap", o, -15, std::vector<Member>(16, {1000, 1048576}));
  }
  inflate_case("P5", def, -16, {{30000, 65536}, {40000, 65536}, {30000, 65536}, {40000, 65536}});
  {
    zs_route_opts o;
    o.inflate_seg = false;
    inflate_case("P6", o, 15, std::vector<Member>(4096, {100000, 262144}));
    o.lane_large_min = 0;
    inflate_case("P6_nolanes", o, 15, std::vector<Member>(4096, {100000, 262144}));
  }
  {
    zs_route_opts o;
    o.seg_scratch_max = 1ull << 20;
    inflate_case("P7", o, 31, std::vector<Member>(16, {20000, 65536}));
  }
  inflate_case("P8", def, -15, std::vector<Member>(2, {300000, 1048576}));
  // the batches of tests/test_gpu_inflate_regions.py: 14 large members (7, each with its output rounded up to 4
  // and with 64 more) and four small ones behind them
  std::vector<Member> few;
  for (const Member& x : {Member{11640, 33004}, {35527, 70004}, {49609, 150004}, {89939, 200004}, {102571, 262144},
                          {25924, 157920}, {70025, 70000}}) {
    few.push_back(x);
    few.push_back({x.in_len, x.out_cap + 64});
  }
  for (const Member& x : {Member{2, 0}, {20, 64}, {2322, 6004}, {3008, 3004}}) few.push_back(x);
  inflate_case("R_few", def, -15, few);
  {
    zs_route_opts o;
    o.seg_split = 1;
    inflate_case("R_few_split1", o, -15, few);
    o = zs_route_opts();
    o.seg_bits = 1024;
    inflate_case("R_few_bits", o, -15, few);
    o = zs_route_opts();
    o.inflate_seg = false;
    o.inflate_wave_min = 1;
    inflate_case("R_wave", o, 15, few);
    o.inflate_ref_wrap = false;
    inflate_case("R_wave_nowrap", o, 31, few);
    inflate_case("R_split_raw", o, -15, few);
    o = zs_route_opts();
    o.inflate_seg = false;
    o.inflate_wave_min = 1024;
    inflate_case("R_nolanes", o, -15, few);
    o.lane_large_min = 1;
    inflate_case("R_lanes", o, -15, few);
  }
  // the three with 64 KiB of input and more on average: the wide window, pieces cut in two
  inflate_case("R_wide", def, -15, std::vector<Member>(few.begin() + 6, few.begin() + 10));
  {
    // 6,001 / 33,002 / 70,003 bytes from about 2 / 12 / 25 KB of input, seg_small_min 256: 520 and 16 of them
    zs_route_opts o;
    o.seg_small_min = 256;
    std::vector<Member> many;
    const Member kinds[3] = {{2322, 6004}, {11640, 33004}, {24960, 70004}};
    for (uint32_t k = 0; k < 520; k++) many.push_back({kinds[k % 3].in_len, kinds[k % 3].out_cap + 64 * ((k / 40) % 2)});
    inflate_case("R520", o, -15, many);
    inflate_case("R520_gzip", o, 31, many);
    many.resize(16);
    inflate_case("R16", o, -15, many);
  }
  // members whose capacity shows a high expansion, a text member beside them
  inflate_case("R_zeros64", def, -16, {{369, 100000}, {369, 100064}, {11640, 33004}});
  inflate_case("R_zeros", def, -15, {{100, 70004}, {454, 262148}, {11640, 33004}});
  {
    zs_route_opts o;
    o.inflate_ref_wrap = false;
    inflate_case("R_zeros_nowrap", o, -15, {{100, 70004}, {454, 262148}, {11640, 33004}});
  }
  deflate_case("D1", def, 6, {100, 65538});
  deflate_case("D_65537", def, 6, {65537});
  deflate_case("D_200000", def, 6, {200000});
  {
    zs_route_opts o;
    o.match_sweep = false;
    deflate_case("D1_nosweep", o, 6, {100, 65538});
  }
  deflate_case("D1_L1", def, 1, {100, 65538});
  deflate_case("PW_2047", def, 6, std::vector<uint32_t>(2047, 16));
  deflate_case("PW_2048", def, 6, std::vector<uint32_t>(2048, 16));
  for (int w : {1, 2, 4}) {
    zs_route_opts o;
    o.parse_waves = w;
    deflate_case(("PW_opt" + std::to_string(w) + "_2047").c_str(), o, 6, std::vector<uint32_t>(2047, 16));
    deflate_case(("PW_opt" + std::to_string(w) + "_2048").c_str(), o, 6, std::vector<uint32_t>(2048, 16));
  }
  return 0;
}
