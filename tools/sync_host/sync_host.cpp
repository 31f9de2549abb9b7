// Runs the restart-point search's per-lane code (zlib-streams-ts_amd/csrc/zs_sync.h: the scan's
// candidate rule over aligned 16-byte units and the count-only decode) on the CPU, one lane at a
// time, from its own source, with the host stand-ins for the HIP names of tools/lane_host; then the
// plan (zs_plan_sync) over the records.  Test tooling: lets the CPU suite check the search without a
// GPU, and a build with -fsanitize=address,undefined shows that no lane leaves the aligned words
// that hold its stream: every stream lies in a buffer of exactly those words.
//
// usage: sync_host WBITS PASS MODE < streams > results
//   stdin:  u32 count, then per stream: u32 in_len, in_len bytes
//   MODE 0: per stream  u32 first, u32 C, C x u32 candidates, (1 + C) x {how, end, len, reach} (the first
//           point's lane, then one per candidate, each bounded by candidate j + PASS + 1), u32 P,
//           P x {in_pos, out_pos} (the points zs_plan_sync emits, the first one included)
//   MODE 1: per stream  u32 first, in_len x {how, end, len, reach}: a lane from EVERY byte offset,
//           bounded by the stream's end
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hip/hip_runtime.h"
zs_dim3 threadIdx, blockIdx, blockDim;
#include "../../zlib-streams-ts_amd/csrc/zs_sync.h"
#define ZS_TOOL "sync_host"
#include "host_stream.h"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int wbits = atoi(argv[1]), mode = atoi(argv[3]);
  const uint32_t pass = (uint32_t)atoi(argv[2]);
  uint32_t count;
  rd(&count, 4);
  static zs_sync_tabs T;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t n;
    rd(&n, 4);
    const HostStream hs(i, n, {0xff, 0xff, 0xff, 0xff});  // (bytes that would show as a candidate, or a header)
    const uint8_t* s = hs.s;
    const uint32_t first = std::min(zs_wrapper_header_len_of(wbits, s, n), n);
    wr(&first, 4);
    if (mode == 1) {
      for (uint32_t at = 0; at < n; at++) {
        const zs_sync_rec r = zs_sync_size(s, n, at, n, T);
        if (r.how < ZS_SYNC_LANDED || r.how > ZS_SYNC_PASSED || r.end > n) {
          fprintf(stderr, "sync_host: stream %u offset %u: a lane ended in no known way\n", i, at);
          return 3;
        }
        wr(&r, 16);
      }
    } else {
      const std::vector<uint32_t> cand = host_scan(s, n, [&](uint64_t u, int64_t& q0) { return zs_sync_unit(s, n, first, u, q0); });
      const uint32_t C = (uint32_t)cand.size();
      std::vector<zs_sync_rec> rec(1 + C);
      const uint64_t cfirst[2] = {0, C};
      for (uint32_t x = 0; x <= C; x++) {
        bool at0;
        const uint32_t bound = host_lane(x, cand, pass, n, at0);
        rec[x] = zs_sync_size(s, n, at0 ? first : cand[x - 1], bound, T);
        if (rec[x].end > bound) {
          fprintf(stderr, "sync_host: stream %u lane %u ended at %u, past its bound %u\n", i, x, rec[x].end, bound);
          return 3;
        }
      }
      zs_sync_plan p;
      zs_plan_sync(1, &n, &first, cfirst, cand.data(), rec.data(), p);
      if (!p.tstream.empty()) {  // a chain that ends at a lane its bound stopped: the whole tail's reach, as sync_batch
        const zs_sync_rec tail = zs_sync_size(s, n, p.tstart[0], n, T, true);
        const uint64_t at = p.trec[0];
        rec[at].reach = std::max(rec[at].reach, tail.reach);
        zs_plan_sync(1, &n, &first, cfirst, cand.data(), rec.data(), p);
      }
      wr(&C, 4);
      wr(cand.data(), 4ull * C);
      wr(rec.data(), 16ull * (1 + C));
      const uint32_t P = (uint32_t)p.rin.size();
      wr(&P, 4);
      for (uint32_t k = 0; k < P; k++) {
        wr(&p.rin[k], 4);
        wr(&p.rout[k], 4);
      }
    }
  }
  return 0;
}
