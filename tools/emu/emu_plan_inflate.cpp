// emu_plan_inflate.cpp -- the fault that wins in an inflate call (csrc/zs_plan.h: zs_inflate_validate for a
// device batch, zs_inflate_validate_host for what a host entry decides before it stages anything), for
// tests/test_plan_inflate_faults.py.  Plain C++, no ROCm headers.
//   g++ -std=c++17 -O2 -o emu_plan_inflate tools/emu/emu_plan_inflate.cpp && ./emu_plan_inflate < cases
// (also as a stand-alone program with -fsanitize=address,undefined)
// A case is a line of stdin (tests/inflatefaultcases.py writes them):
//   name ctx wbits n dict arrays buf lens offs caps
// ctx: a context is given; dict: the entry takes dictionaries; arrays / buf: their offsets and lengths /
// their bytes are given; lens, offs, caps: n values each, separated by commas ("-": none).  Printed per
// case, separated by tabs: the name, then index and text of the device and of the host verdict.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../../zlib-streams-ts_amd/csrc/zs_plan.h"

template <class T>
static std::vector<T> list(const char* s, size_t n) {
  std::vector<T> v;
  for (const char* p = s; *p && *p != '-';) {
    char* end;
    v.push_back((T)strtoull(p, &end, 10));
    p = *end == ',' ? end + 1 : end;
  }
  if (v.size() != n) {
    fprintf(stderr, "a list of %zu values, not of %zu: %s\n", v.size(), n, s);
    exit(2);
  }
  return v;
}

int main() {
  char name[128], lens[256], offs[256], caps[256];
  int ctx, wbits, dict, arrays, buf;
  unsigned n;
  while (scanf("%127s %d %d %u %d %d %d %255s %255s %255s", name, &ctx, &wbits, &n, &dict, &arrays, &buf, lens, offs, caps) ==
         10) {
    const std::vector<uint32_t> dl = list<uint32_t>(lens, n), oc = list<uint32_t>(caps, n);
    const std::vector<uint64_t> oo = list<uint64_t>(offs, n);
    zs_inflate_call a;
    a.n = n;
    a.out_cap = oc.data();
    a.dict = dict != 0;
    a.dict_arrays = dict && arrays;
    a.dict_buf = dict && buf;
    a.dict_len = a.dict_arrays ? dl.data() : nullptr;
    // the device entries: the caller's regions
    a.out_off = oo.data();
    a.caller_regions = true;
    const zs_inflate_err dev = zs_inflate_validate(ctx != 0, wbits, a);
    // the host entries: the staging's own
    a.out_off = nullptr;
    a.caller_regions = false;
    const zs_inflate_err host = zs_inflate_validate_host(ctx != 0, wbits, a);
    printf("%s\t%d\t%s\t%d\t%s\n", name, (int)dev, zs_inflate_err_text(dev), (int)host, zs_inflate_err_text(host));
  }
  return 0;
}
