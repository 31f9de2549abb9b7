// emu_plan_bgzf_range.cpp -- what csrc/zs_plan.h decides for a batch of BGZF ranges by virtual offset
// (zs_bgzf_range_validate, zs_bgzf_range_slice, zs_plan_bgzf_range), printed one line of key=value pairs per
// stream and per case for tests/test_plan_bgzf_range.py.  The records of the slices' starts come from the
// test, which reads them from the headers of real files by the rule of include/zs_gpu.h.  Plain C++, no ROCm
// headers.
//   g++ -std=c++17 -O2 -o emu_plan_bgzf_range tools/emu/emu_plan_bgzf_range.cpp && ./emu_plan_bgzf_range < cases
// (also as a stand-alone program with -fsanitize=address,undefined)
// stdin, text:  per case   "case NAME n"
//               per stream "stream in_len out_cap vb ve C", then 1 + C lines "pos how end len trusted": the
//               slice's offset 0 first, then its candidates in increasing order
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"

template <class T>
static std::string list(const std::vector<T>& v, size_t a, size_t b) {
  std::string s;
  for (size_t i = a; i < b; i++) s += (i > a ? "," : "") + std::to_string(v[i]);
  return s.empty() ? "-" : s;
}

int main() {
  char name[256];
  unsigned n;
  while (scanf(" case %255s %u", name, &n) == 2) {
    std::vector<uint32_t> in_len(n), out_cap(n), cand;
    std::vector<uint64_t> vb(n), ve(n), cfirst(n + 1, 0);
    std::vector<zs_sync_rec> rec0(n), recc;
    std::vector<uint8_t> t0(n), tc;
    for (unsigned i = 0; i < n; i++) {
      unsigned long long b, e;
      unsigned len, cap, C;
      if (scanf(" stream %u %u %llu %llu %u", &len, &cap, &b, &e, &C) != 5) return 2;
      in_len[i] = len;
      out_cap[i] = cap;
      vb[i] = b;
      ve[i] = e;
      for (unsigned k = 0; k <= C; k++) {
        unsigned pos, how, end, l, t;
        if (scanf(" %u %u %u %u %u", &pos, &how, &end, &l, &t) != 5) return 2;
        const zs_sync_rec r = {how, end, l, 0u};
        if (k == 0) {
          if (pos != 0) return 2;
          rec0[i] = r;
          t0[i] = (uint8_t)t;
        } else {
          cand.push_back(pos);
          recc.push_back(r);
          tc.push_back((uint8_t)t);
        }
      }
      cfirst[i + 1] = cand.size();
    }
    const zs_bgzf_range_err e = zs_bgzf_range_validate(n, in_len.data(), vb.data(), ve.data());
    if (e != ZS_BR_OK) {
      printf("case=%s refused=%d\n", name, (int)e);
      continue;
    }
    std::vector<zs_sync_rec> rec(rec0);
    rec.insert(rec.end(), recc.begin(), recc.end());
    std::vector<uint8_t> rt(t0);
    rt.insert(rt.end(), tc.begin(), tc.end());
    zs_bgzf_range_plan p;
    zs_plan_bgzf_range(n, out_cap.data(), vb.data(), ve.data(), cfirst.data(), cand.data(), rec.data(), rt.data(), p);
    for (unsigned i = 0; i < n; i++) {
      uint32_t off, len;
      zs_bgzf_range_slice(in_len[i], vb[i], ve[i], off, len);
      const size_t a = p.rfirst[i], b = p.rfirst[i + 1];
      std::vector<uint32_t> tr(p.trusted.begin(), p.trusted.end());
      printf("case=%s/%u slice_off=%u slice_len=%u verdict=%u vcons=%u soff=%s slen=%s ocap=%s skip=%s take=%s opos=%s "
             "trusted=%s stoff=%s\n",
             name, i, off, len, p.verdict[i], p.vcons[i], list(p.soff, a, b).c_str(), list(p.slen, a, b).c_str(),
             list(p.ocap, a, b).c_str(), list(p.skip, a, b).c_str(), list(p.take, a, b).c_str(), list(p.opos, a, b).c_str(),
             list(tr, a, b).c_str(), list(p.stoff, a, b).c_str());
    }
    printf("case=%s refused=0 M=%u rstream=%s ptile=%s stage=%llu\n", name, p.M, list(p.rstream, 0, p.M).c_str(),
           list(p.ptile, 0, p.ptile.size()).c_str(), (unsigned long long)p.stage_bytes);
  }
  return 0;
}
