// Runs the member search's per-lane code (zlib-streams-ts_amd/csrc/zs_members.h: the scan's candidate
// rule over aligned 16-byte units and the sizing of one member) on the CPU, one lane at a time, from
// its own source, with the host stand-ins for the HIP names of tools/lane_host; then the plan
// (zs_plan_members) over the records, with its tail rounds.  Test tooling: lets the CPU suite check the
// search without a GPU, and a build with -fsanitize=address,undefined shows that no lane leaves the
// aligned words that hold its stream: every stream lies in a buffer of exactly those words.
//
// usage: members_host PASS MODE < streams > results
//   stdin:  u32 count, then per stream: u32 in_len, u32 out_cap, in_len bytes
//   MODE 0: per stream  u32 C, C x u32 candidates, (1 + C) x {how, end, len, reach} (offset 0's lane, then
//           one per candidate, each bounded by candidate j + PASS + 1), u32 tail rounds, u32 in_place,
//           u32 P, P x {in_pos, in_len, out_pos, cap} (the members zs_plan_members emits)
//   MODE 1: per stream  in_len x {how, end, len, reach}: a lane from EVERY byte offset, bounded by the
//           stream's end
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hip/hip_runtime.h"
zs_dim3 threadIdx, blockIdx, blockDim;
#include "../../zlib-streams-ts_amd/csrc/zs_members.h"
#define ZS_TOOL "members_host"
#include "host_stream.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint32_t pass = (uint32_t)atoi(argv[1]);
  const int mode = atoi(argv[2]);
  uint32_t count;
  rd(&count, 4);
  static zs_sync_tabs T;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t n, out_cap;
    rd(&n, 4);
    rd(&out_cap, 4);
    const HostStream hs(i, n, {0x1f, 0x8b, 0x08, 0x00});  // (bytes that would show as a candidate, or a header)
    const uint8_t* s = hs.s;
    if (mode == 1) {
      for (uint32_t at = 0; at < n; at++) {
        const zs_sync_rec r = zs_members_size(s, n, at, n, T);
        if ((r.how != ZS_SYNC_FINAL && r.how != ZS_SYNC_ERROR) || r.end > n) {
          fprintf(stderr, "members_host: stream %u offset %u: an unbounded lane ended in no known way\n", i, at);
          return 3;
        }
        wr(&r, 16);
      }
    } else {
      const std::vector<uint32_t> cand = host_scan(s, n, [&](uint64_t u, int64_t& q0) { return zs_members_unit(s, n, u, q0); });
      const uint32_t C = (uint32_t)cand.size();
      std::vector<zs_sync_rec> rec(1 + C);
      const uint64_t cfirst[2] = {0, C};
      for (uint32_t x = 0; x <= C; x++) {
        bool at0;
        const uint32_t bound = host_lane(x, cand, pass, n, at0);
        rec[x] = zs_members_size(s, n, at0 ? 0u : cand[x - 1], bound, T);
        if (rec[x].end > bound) {
          fprintf(stderr, "members_host: stream %u lane %u ended at %u, past its bound %u\n", i, x, rec[x].end, bound);
          return 3;
        }
      }
      wr(&C, 4);
      wr(cand.data(), 4ull * C);
      wr(rec.data(), 16ull * (1 + C));
      zs_members_plan p;
      uint32_t rounds = 0;
      for (;; rounds++) {  // the tail rounds, as members_batch runs them
        zs_plan_members(1, &n, &out_cap, cfirst, cand.data(), rec.data(), p);
        if (p.tstream.empty()) break;
        if (rounds > C) {
          fprintf(stderr, "members_host: stream %u: the tail rounds do not end\n", i);
          return 3;
        }
        for (size_t k = 0; k < p.tstream.size(); k++) rec[p.trec[k]] = zs_members_size(s, n, p.tstart[k], n, T);
      }
      const uint32_t P = p.M, inp = p.in_place;
      wr(&rounds, 4);
      wr(&inp, 4);
      wr(&P, 4);
      for (uint32_t k = 0; k < P; k++) {
        wr(&p.soff[k], 4);
        wr(&p.slen[k], 4);
        wr(&p.opos[k], 4);
        wr(&p.ocap[k], 4);
      }
    }
  }
  return 0;
}
