// emu_plan_restart.cpp -- what csrc/zs_plan.h decides for an inflate batch with restart points: the
// validation order (zs_restart_validate), the segments, their copies' places in the gather buffer,
// their output places and capacities, the route (zs_plan_restart), the call's section of the metadata
// block (zs_section_put over the plan's arrays) and the segment batch's own plan (zs_plan_inflate over the copies'
// lengths), printed one line of key=value pairs per case for tests/test_plan_restart.py.  Plain C++,
// no ROCm headers.
//   g++ -std=c++17 -O2 -o emu_plan_restart tools/emu/emu_plan_restart.cpp && ./emu_plan_restart
// (also as a stand-alone program with -fsanitize=address,undefined)
#include <stdio.h>

#include <string>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"

template <class T>
static std::string list(const std::vector<T>& v) {
  std::string s;
  for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
  return s.empty() ? "-" : s;
}

struct Call {
  std::vector<uint32_t> len, cap;   // the streams' input lengths and output capacities
  std::vector<uint64_t> first;
  std::vector<uint32_t> rin, rout;  // the points, the first one of every stream included
  std::vector<uint64_t> out_off;
  zs_restart_call call(bool device = true) {
    out_off.assign(len.size(), 0);
    for (size_t i = 1; i < len.size(); i++) out_off[i] = out_off[i - 1] + ((cap[i - 1] + 3) & ~3u);
    zs_restart_call a;
    a.n = (uint32_t)len.size();
    a.in_len = len.data();
    a.out_off = device ? out_off.data() : nullptr;
    a.out_cap = cap.data();
    a.caller_regions = device;
    a.rfirst = first.data();
    a.rin = rin.data();
    a.rout = rout.data();
    return a;
  }
};

static void print_inflate(const char* name, const zs_inflate_plan& p) {
  printf("case=%s seg=%s split=%s wave=%s wave_min=%u block=%u rt=%d piece_cap=%u val_stride=%llu refw=%d lanes=%d\n", name,
         list(p.seg).c_str(), list(p.split).c_str(), list(p.wave).c_str(), p.wave_min, p.lane.block, p.lane.rt, p.piece_cap,
         (unsigned long long)p.val_stride, (int)p.wave_refw, (int)p.wave_lanes);
}

static void segments(const char* name, int wbits, Call c) {
  zs_restart_call a = c.call();
  const int valid = (int)zs_restart_validate(wbits, a);
  zs_restart_plan p;
  zs_plan_restart(a.n, a.in_len, a.out_cap, a.rfirst, a.rin, a.rout, p);
  const zs_meta_layout ml(p.M);
  // the call's section as restart_batch writes it behind the segment batch's block: the streams' arrays first
  std::vector<uint8_t> sec;
  const size_t s_in_off = zs_section_put(sec, nullptr, 8ull * a.n);
  zs_section_put(sec, a.in_len, 4ull * a.n);
  zs_section_put(sec, p.soff.data(), 4ull * p.M);
  const size_t s_ptile = zs_section_put(sec, p.ptile.data(), 4ull * (p.M + 1));
  int aligned = 1, apart = 1, staged = 1;
  for (uint32_t g = 0; g < p.M; g++) {
    aligned &= (p.goff[g] & 15) == 0;
    // a copy, its 03 00 and its zero padding to a whole aligned word end before the next copy starts
    const uint64_t end = p.goff[g] + ((p.glen[g] + 3ull) & ~3ull);
    apart &= end <= (g + 1 < p.M ? p.goff[g + 1] : p.gather_bytes);
    staged &= (p.stoff[g] & 3) == 0 && (g + 1 == p.M || p.stoff[g] + ((p.ocap[g] + 3ull) & ~3ull) <= p.stoff[g + 1]);
  }
  printf("case=seg/%s valid=%d M=%u in_place=%d rfirst=%s rstream=%s soff=%s slen=%s glen=%s goff=%s opos=%s olen=%s "
         "ocap=%s stoff=%s over=%s gtile=%s ptile=%s gather=%llu stage=%llu aligned=%d apart=%d staged=%d meta_after=%d\n",
         name, valid, p.M, (int)p.in_place, list(p.rfirst).c_str(), list(p.rstream).c_str(), list(p.soff).c_str(),
         list(p.slen).c_str(), list(p.glen).c_str(), list(p.goff).c_str(), list(p.opos).c_str(), list(p.olen).c_str(),
         list(p.ocap).c_str(), list(p.stoff).c_str(), list(p.over).c_str(), list(p.gtile).c_str(), list(p.ptile).c_str(),
         (unsigned long long)p.gather_bytes, (unsigned long long)p.stage_bytes, aligned, apart, staged,
         (int)(s_in_off == 0 && sec.size() > s_ptile && (ml.bytes + sec.size()) % 256 == 0));
}

static void refusal(const char* name, int wbits, Call c, int nulls = 0, bool misalign = false) {
  zs_restart_call dev = c.call(true), host = c.call(false);
  if (misalign) c.out_off[0] = 2;  // (the host entries stage their own regions: they never see it)
  for (zs_restart_call* a : {&dev, &host}) {
    if (nulls & 1) a->rfirst = nullptr;
    if (nulls & 2) a->rin = nullptr;
    if (nulls & 4) a->rout = nullptr;
  }
  printf("case=refuse/%s device=%d host=%d\n", name, (int)zs_restart_validate(wbits, dev), (int)zs_restart_validate(wbits, host));
}

int main() {
  char name[64];
  // one point: the plain stream, one segment that ends by itself
  segments("one", 15, {{100}, {400}, {0, 1}, {2}, {0}});
  // points at 0 and at the end of the output: a marker alone, a last segment of 03 00 and the trailer
  segments("ends", 15, {{23}, {8}, {0, 3}, {2, 7, 17}, {0, 0, 3}});
  // b"abc" with every subset of the flush positions {0, 1, 2, 3}: in_pos as zlib's level 6 gives them
  // (every piece of one byte: a fixed block of 3 bytes, then the marker's 5), raw
  for (int m = 0; m < 16; m++) {
    Call c{{0}, {4}, {0, 1}, {0}, {0}};
    uint32_t in = 0, at = 0;
    for (uint32_t b = 0; b < 4; b++)
      if (m >> b & 1) {
        in += (b > at ? b - at + 2 : 0) + 5;
        at = b;
        c.rin.push_back(in);
        c.rout.push_back(b);
      }
    c.first[1] = c.rin.size();
    c.len[0] = in + (3 > at ? 3 - at + 2 : 2);
    snprintf(name, sizeof name, "abc/%d", m);
    segments(name, -15, c);
  }
  // in place: every restart out_pos a multiple of 4 -- and not as soon as one point of the call is none
  segments("in_place", 31, {{300, 200}, {1000, 1000}, {0, 3, 5}, {10, 100, 200, 10, 150}, {0, 400, 800, 0, 4}});
  segments("staged", 31, {{300, 200}, {1000, 1000}, {0, 3, 5}, {10, 100, 200, 10, 150}, {0, 400, 800, 0, 5}});
  // capacities: a stream whose last point lies past its capacity, segments cut at it
  segments("over", -15, {{300}, {500}, {0, 3}, {0, 100, 200}, {0, 400, 800}});
  // a 300-byte and a 1 MiB segment in one call: one tile and 257
  segments("tiles", -15, {{300 + (1u << 20)}, {4u << 20}, {0, 2}, {0, 300}, {0, 1000}});
  // a call with only first points plans the segment batch as zs_plan_inflate plans the same lengths
  {
    Call c{{0, 1, 100, 5000, 40000, 300000}, {4, 4, 400, 20000, 160000, 1200000}, {0, 1, 2, 3, 4, 5, 6}, {0, 0, 0, 0, 0, 0},
           {0, 0, 0, 0, 0, 0}};
    zs_restart_call a = c.call();
    zs_restart_plan p;
    zs_plan_restart(a.n, a.in_len, a.out_cap, a.rfirst, a.rin, a.rout, p);
    zs_route_opts o;
    o.inflate_ref_wrap = false;
    zs_inflate_plan viaseg, direct;
    zs_plan_inflate(o, -15, p.M, p.glen.data(), p.ocap.data(), viaseg);
    zs_plan_inflate(o, -15, a.n, a.in_len, a.out_cap, direct);
    print_inflate("first_only/segments", viaseg);
    print_inflate("first_only/direct", direct);
    printf("case=first_only/plan M=%u in_place=%d glen=%s ocap=%s\n", p.M, (int)p.in_place, list(p.glen).c_str(),
           list(p.ocap).c_str());
  }
  // every refusal, in validation order
  const Call ok{{100, 50}, {400, 200}, {0, 2, 3}, {2, 40, 2}, {0, 100, 0}};
  refusal("ok", 15, ok);
  refusal("d64", -16, ok, 7);   // the format first, whatever else is wrong
  refusal("wbits", 14, ok, 7);
  refusal("wbits0", 0, ok);
  refusal("null_first", 15, ok, 1);
  refusal("null_in", 15, ok, 2);
  refusal("null_out", 15, ok, 4);
  refusal("empty_batch", 15, {{}, {}, {0}, {}, {}}, 7);
  refusal("no_first", 15, {{100, 50}, {400, 200}, {0, 2, 2}, {2, 40}, {0, 100}});
  refusal("first_decreasing", 15, {{100, 50}, {400, 200}, {2, 0, 2}, {2, 40}, {0, 100}});
  refusal("many", 15, {{100}, {400}, {0, (uint64_t)ZS_RESTART_SEG_MAX + 1}, {2}, {0}});  // (the count alone: no point is read)
  refusal("first_out", 15, {{100, 50}, {400, 200}, {0, 2, 3}, {2, 40, 2}, {0, 100, 1}});
  refusal("in_equal", 15, {{100}, {400}, {0, 2}, {2, 2}, {0, 100}});
  refusal("in_gap4", 15, {{100}, {400}, {0, 3}, {2, 7, 11}, {0, 0, 50}});
  refusal("in_gap5", 15, {{100}, {400}, {0, 3}, {2, 7, 12}, {0, 0, 50}});
  refusal("in_decreasing", 15, {{100}, {400}, {0, 3}, {2, 40, 20}, {0, 10, 50}});
  refusal("out_decreasing", 15, {{100}, {400}, {0, 3}, {2, 40, 60}, {0, 100, 99}});
  refusal("out_equal", 15, {{100}, {400}, {0, 3}, {2, 40, 60}, {0, 100, 100}});
  refusal("past_end", 15, {{100}, {400}, {0, 2}, {2, 101}, {0, 100}});
  refusal("at_end", 15, {{100}, {400}, {0, 2}, {2, 100}, {0, 100}});
  refusal("first_past_end", 31, {{9}, {400}, {0, 1}, {10}, {0}});
  // the order: in_pos before out_pos before the length, at one point; a stream's faults in stream order
  refusal("in_then_out", 15, {{100}, {400}, {0, 2}, {2, 3}, {0, 0}});
  refusal("in_before_past_end", 15, {{100}, {400}, {0, 3}, {2, 200, 201}, {0, 10, 5}});
  refusal("out_before_past_end", 15, {{100}, {400}, {0, 3}, {2, 40, 200}, {0, 10, 5}});
  refusal("stream_order", 15, {{100, 50}, {400, 200}, {0, 2, 4}, {2, 101, 2, 3}, {0, 100, 1, 0}});
  refusal("align", 15, ok, 0, true);  // the device entry's rule, after the points
  refusal("align_after_points", 15, {{100}, {400}, {0, 2}, {2, 2}, {0, 100}}, 0, true);
  {
    Call c = ok;
    c.cap[1] = 202;
    refusal("align_cap", 15, c);
  }
  return 0;
}
