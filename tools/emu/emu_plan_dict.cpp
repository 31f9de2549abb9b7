// emu_plan_dict -- prints what csrc/zs_plan.h decides for batches whose members
// have preset dictionaries, and what csrc/zs_dict.h lays out for the host entries
// (the distinct dictionaries, their packed staging), one line of key=value pairs
// per case (tests/test_plan_dict.py holds the expected values).  Host only:
// g++ -std=c++17 -O2 -Wall -Werror, no ROCm headers; the test also builds it with
// -fsanitize=address,undefined.
#include <stdio.h>

#include <string>

#include "../../zlib-streams-ts_amd/csrc/zs_dict.h"
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
  uint32_t in_len, out_cap, dict_len;
};

static void plan_case(const char* name, const zs_route_opts& o, int wbits, const std::vector<Member>& m) {
  std::vector<uint32_t> in_len, out_cap, dict_len;
  for (const Member& x : m) {
    in_len.push_back(x.in_len);
    out_cap.push_back(x.out_cap);
    dict_len.push_back(x.dict_len);
  }
  zs_inflate_plan p, q;
  zs_plan_inflate(o, wbits, (uint32_t)m.size(), in_len.data(), out_cap.data(), p, dict_len.data());
  zs_plan_inflate(o, wbits, (uint32_t)m.size(), in_len.data(), out_cap.data(), q);  // the same batch without them
  printf("case=%s n=%zu dict=%d dict_lane=%s dict_exact=%s seg=%s split=%s wave=%s wave_min=%u lane_block=%u "
         "lane_rt=%d nodict_seg=%s nodict_split=%s nodict_wave=%s nodict_lane_block=%u\n",
         name, m.size(), (int)p.dict, ranges(p.dict_lane).c_str(), ranges(p.dict_exact).c_str(), ranges(p.seg).c_str(),
         ranges(p.split).c_str(), ranges(p.wave).c_str(), p.wave_min, p.lane.block, p.lane.rt, ranges(q.seg).c_str(),
         ranges(q.split).c_str(), ranges(q.wave).c_str(), q.lane.block);
}

struct Dict {
  uint64_t off;
  uint32_t len;
};

// the distinct dictionaries, the packed staging and its bytes (a checksum of them)
static void layout_case(const char* name, const std::vector<Dict>& m, uint64_t src_bytes) {
  std::vector<uint64_t> off, upos, poff;
  std::vector<uint32_t> len;
  for (const Dict& x : m) {
    off.push_back(x.off);
    len.push_back(x.len);
  }
  std::vector<uint8_t> src(src_bytes);
  for (uint64_t i = 0; i < src_bytes; i++) src[i] = (uint8_t)(i * 7 + (i >> 8));
  zs_dict_set d;
  zs_dict_distinct((uint32_t)m.size(), off.data(), len.data(), d);
  const uint64_t total = zs_dict_pack_layout(d, (uint32_t)m.size(), len.data(), upos, poff);
  std::vector<uint8_t> pack(total);
  zs_dict_pack(d, upos, src.data(), pack.data());
  // every member's packed bytes are its own
  int same = 1;
  for (size_t i = 0; i < m.size(); i++)
    for (uint32_t k = 0; k < len[i]; k++) same &= pack[poff[i] + k] == src[off[i] + k];
  printf("case=%s n=%zu any=%d distinct=%zu total=%llu same=%d id=", name, m.size(), (int)d.any, d.uoff.size(),
         (unsigned long long)total, same);
  for (size_t i = 0; i < m.size(); i++) printf("%s%u", i ? "," : "", d.id[i]);
  printf(" poff=");
  for (size_t i = 0; i < m.size(); i++) printf("%s%llu", i ? "," : "", (unsigned long long)poff[i]);
  printf("\n");
}

int main() {
  const zs_route_opts def;
  // 64 single-call members sharing a dictionary
  plan_case("shared64", def, -15, std::vector<Member>(64, {1500, 4096, 32768}));
  // a 40,000-byte input: past one 32 KiB sub-chunk
  plan_case("in40000", def, 15, {{1500, 4096, 257}, {40000, 65536, 257}, {1500, 4096, 257}});
  // capacities around 64 KiB, inputs around 32 KiB
  plan_case("edges", def, -15, {{32768, 65536, 1}, {32769, 65536, 1}, {32768, 65540, 1}, {100, 4, 1}});
  // a small batch (the segmented decode takes members over 4 KiB of input): dictionary members stay out of it,
  // the members without a dictionary keep their routes
  plan_case("mixed_small", def, -15,
            {{20000, 65536, 100}, {20000, 65536, 0}, {90000, 262144, 100}, {90000, 262144, 0}, {1000, 1048576, 5},
             {1000, 1048576, 0}, {100, 1024, 0}, {100, 1024, 7}});
  {
    zs_route_opts o;
    o.inflate_ref_wrap = false;  // raw members are splittable: the high-expansion one without a dictionary
    plan_case("mixed_nowrap", o, -15, {{1000, 1048576, 5}, {1000, 1048576, 0}, {300000, 1048576, 9}});
    o.inflate_seg = false;
    plan_case("mixed_noseg", o, 15, {{90000, 262144, 100}, {90000, 262144, 0}, {100, 1024, 100}});
  }
  // dict_len all zero: the plan of a batch without dictionaries
  plan_case("all_zero", def, 15, {{20000, 65536, 0}, {100, 1024, 0}});
  plan_case("large_batch", def, 15, std::vector<Member>(65536, {1500, 4096, 32768}));

  layout_case("one_shared", std::vector<Dict>(5, {3, 1000}), 1003);
  layout_case("three_aliased", {{1, 10}, {0, 0}, {11, 300}, {1, 10}, {11, 299}, {11, 300}, {999, 0}}, 311);
  layout_case("none", {{5, 0}, {0, 0}}, 0);
  layout_case("overlapping", {{0, 8}, {4, 8}, {0, 12}}, 12);
  return 0;
}
