// Runs the dictionary instances of the lane-per-member inflate kernel
// (zs_k_inflate_lane<., false, true>, zlib-streams-ts_amd/csrc/inflate_lane.hip) on
// the CPU, one member at a time, from the kernel's own source -- lane_host's
// companion for members with a preset dictionary.  Test tooling.
//
// The three instances (canonical decode only, root tables, root tables with the
// canonical limits in LDS) run on every member and must agree.
//
// usage: lane_dict_host WBITS FLAGS < members > results
//   stdin:  u32 count, then per member: u32 in_len, u32 out_cap, u32 dict_len,
//           in_len bytes, dict_len bytes
//   stdout: per member: u32 bail, u32 out_len, u32 consumed, u32 want, out_len bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hip/hip_runtime.h"  // (tools/lane_host/hip: the host stand-ins)
zs_dim3 threadIdx, blockIdx, blockDim;
#include "../../zlib-streams-ts_amd/csrc/inflate_lane.hip"
alignas(16) uint8_t LL[sizeof(zs_lane_lds_root)];

static void rd(void* p, size_t n) {
  if (fread(p, 1, n, stdin) != n) {
    fprintf(stderr, "lane_dict_host: short input\n");
    exit(2);
  }
}
static uint32_t adler32(const uint8_t* p, size_t n) {
  uint32_t a = 1, b = 0;
  for (size_t i = 0; i < n; i++) {
    a = (a + p[i]) % 65521u;
    b = (b + a) % 65521u;
  }
  return (b << 16) | a;
}
struct Run {
  zs_lane_res r;
  std::vector<uint8_t> out;
};
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int wbits = atoi(argv[1]), flags = atoi(argv[2]);
  uint32_t n;
  rd(&n, 4);
  for (uint32_t i = 0; i < n; i++) {
    uint32_t len, cap, dlen;
    rd(&len, 4);
    rd(&cap, 4);
    rd(&dlen, 4);
    // 16-byte aligned buffers with slack, as device allocations are; member and
    // dictionary start at varying misalignments (the dictionary: any byte offset).
    // The dictionary ends 3 bytes before its buffer's end: the words the kernel may
    // read reach no further (AddressSanitizer checks that in the -fsanitize build).
    const uint32_t mis = i % 16, dmis = (i * 7 + 1) % 16;
    std::vector<uint4> ib((len + mis + 64) / 16 + 1), ob((cap + mis + 64) / 16 + 1);
    uint8_t* in = (uint8_t*)ib.data();
    rd(in + mis, len);
    const uint32_t dpad = (4u - (dmis + dlen) % 4u) % 4u;  // to the end of the last word
    uint8_t* db = (uint8_t*)malloc(dmis + dlen + dpad + 4);  // (malloc: 16-aligned)
    if (!db) return 2;
    db += 4;  // ... and it starts within a word of its buffer's start
    rd(db + dmis, dlen);
    uint64_t ioff = mis, ooff = ((i * 5) % 16) & ~3u, doff = dmis;
    const uint32_t did = 0, dad = adler32(db + dmis, dlen);
    const zs_dict_args dd = {db, &doff, &dlen, &did, &dad};
    uint32_t lo;
    threadIdx = {0, 0, 0};
    blockIdx = {0, 0, 0};
    blockDim = {1, 1, 1};
    std::vector<zs_lane_tabs> tabs(1);
    uint8_t* ob8 = (uint8_t*)ob.data();
    const size_t obn = ob.size() * sizeof(uint4);
    Run runs[3];
    for (int v = 0; v < 3; v++) {
      for (size_t k = 0; k < obn; k++) ob8[k] = 0xa5;  // guard pattern around the member's output
      zs_lane_res& r = runs[v].r;
      if (v == 0)
        zs_k_inflate_lane<0, false, true>(in, &ioff, &len, ob8, &ooff, &cap, wbits, 1, tabs.data(), &r, &lo, flags, 0u,
                                          nullptr, dd);
      else if (v == 1)
        zs_k_inflate_lane<1, false, true>(in, &ioff, &len, ob8, &ooff, &cap, wbits, 1, tabs.data(), &r, &lo, flags, 0u,
                                          nullptr, dd);
      else
        zs_k_inflate_lane<2, false, true>(in, &ioff, &len, ob8, &ooff, &cap, wbits, 1, tabs.data(), &r, &lo, flags, 0u,
                                          nullptr, dd);
      runs[v].out.assign(ob8, ob8 + obn);
      for (size_t k = 0; k < obn; k++)
        if ((k < ooff || k >= ooff + cap) && ob8[k] != 0xa5) {
          fprintf(stderr, "lane_dict_host: member %u wrote byte %zu outside [%lu, %lu)\n", i, k, (unsigned long)ooff,
                  (unsigned long)(ooff + cap));
          exit(3);
        }
      const zs_lane_res& a = runs[0].r;
      if (r.bail != a.bail || (!r.bail && (r.out_len != a.out_len || r.consumed != a.consumed || r.want != a.want ||
                                           memcmp(ob8 + ooff, runs[0].out.data() + ooff, r.out_len)))) {
        fprintf(stderr, "lane_dict_host: member %u: instance %d differs from the canonical decoder\n", i, v);
        exit(4);
      }
    }
    const zs_lane_res& r = runs[0].r;
    fwrite(&r, 4, 4, stdout);
    fwrite(runs[0].out.data() + ooff, 1, r.bail ? 0 : r.out_len, stdout);
    free(db - 4);
  }
  return 0;
}
