// emu_plan_members.cpp -- what csrc/zs_plan.h decides for an inflate batch that finds its gzip members:
// the members zs_plan_members lays out from the candidates and the lanes' records (the chain, the
// capacity cut, the in-place and the staged route, the tail list) and the validation order
// (zs_members_validate), for tests/test_plan_members.py.  Plain C++, no ROCm headers.
//   g++ -std=c++17 -O2 -o emu_plan_members tools/emu/emu_plan_members.cpp && ./emu_plan_members < cases
// Lines of stdin:
//   plan NAME STREAMS   STREAMS: streams separated by '/', each  in_len:out_cap:cands:recs  with cands a comma
//                       list ("-": none) and recs 1 + C records how.end.len.reach, comma separated (offset
//                       0's lane, then one per candidate)
//        -> case=NAME first=... stream=... in=... len=... out=... cap=... stoff=... ptile=... in_place=0|1
//           stage=BYTES tstream=... tstart=... trec=...
//   validate NAME WBITS N CAPS OFFS   CAPS / OFFS: N values each ("-": null)
//        -> case=NAME device=E host=E text=... (zs_members_err of the device and of the host entry)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"

static std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  size_t at = 0;
  for (;;) {
    const size_t e = s.find(sep, at);
    out.push_back(s.substr(at, e == std::string::npos ? e : e - at));
    if (e == std::string::npos) break;
    at = e + 1;
  }
  return out;
}
template <class T>
static std::vector<T> nums(const std::string& s, char sep = ',') {
  std::vector<T> v;
  if (s == "-" || s.empty()) return v;
  for (const std::string& x : split(s, sep)) v.push_back((T)strtoull(x.c_str(), nullptr, 10));
  return v;
}
template <class T>
static std::string list(const std::vector<T>& v) {
  std::string s;
  for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
  return s.empty() ? "-" : s;
}

int main() {
  static char kind[32], name[128], a[4096], b[1 << 20], c[1 << 20];
  while (scanf("%31s %127s", kind, name) == 2) {
    if (!strcmp(kind, "plan")) {
      if (scanf("%1048575s", c) != 1) return 2;
      std::vector<uint32_t> in_len, out_cap, cand;
      std::vector<uint64_t> cfirst(1, 0);
      std::vector<zs_sync_rec> firsts, cands;
      for (const std::string& st : split(c, '/')) {
        const std::vector<std::string> f = split(st, ':');
        if (f.size() != 4) return 2;
        in_len.push_back((uint32_t)strtoull(f[0].c_str(), nullptr, 10));
        out_cap.push_back((uint32_t)strtoull(f[1].c_str(), nullptr, 10));
        const std::vector<uint32_t> cs = nums<uint32_t>(f[2]);
        cand.insert(cand.end(), cs.begin(), cs.end());
        cfirst.push_back(cand.size());
        const std::vector<std::string> rs = split(f[3], ',');
        if (rs.size() != cs.size() + 1) return 2;
        for (size_t k = 0; k < rs.size(); k++) {
          const std::vector<uint32_t> v = nums<uint32_t>(rs[k], '.');
          if (v.size() != 4) return 2;
          (k ? cands : firsts).push_back({v[0], v[1], v[2], v[3]});
        }
      }
      std::vector<zs_sync_rec> rec = firsts;
      rec.insert(rec.end(), cands.begin(), cands.end());
      zs_members_plan p;
      zs_plan_members((uint32_t)in_len.size(), in_len.data(), out_cap.data(), cfirst.data(), cand.data(), rec.data(), p);
      printf("case=%s first=%s stream=%s in=%s len=%s out=%s cap=%s stoff=%s ptile=%s in_place=%d stage=%llu tstream=%s "
             "tstart=%s trec=%s\n",
             name, list(p.rfirst).c_str(), list(p.rstream).c_str(), list(p.soff).c_str(), list(p.slen).c_str(),
             list(p.opos).c_str(), list(p.ocap).c_str(), list(p.stoff).c_str(), list(p.ptile).c_str(), (int)p.in_place,
             (unsigned long long)p.stage_bytes, list(p.tstream).c_str(), list(p.tstart).c_str(), list(p.trec).c_str());
    } else if (!strcmp(kind, "validate")) {
      int wbits, n;
      if (scanf("%d %d %4095s %1048575s", &wbits, &n, a, b) != 4) return 2;
      const std::vector<uint32_t> caps = nums<uint32_t>(a);
      const std::vector<uint64_t> offs = nums<uint64_t>(b);
      zs_inflate_call dev, host;
      dev.n = host.n = (uint32_t)n;
      dev.out_cap = host.out_cap = strcmp(a, "-") ? caps.data() : nullptr;
      dev.out_off = strcmp(b, "-") ? offs.data() : nullptr;
      dev.caller_regions = true;
      const zs_members_err d = zs_members_validate(wbits, dev), h = zs_members_validate(wbits, host);
      printf("case=%s device=%d host=%d text=%s\n", name, (int)d, (int)h, zs_members_err_text(d));
    } else {
      return 2;
    }
  }
  return 0;
}
