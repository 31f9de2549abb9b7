// Runs the BGZF fast path's per-lane code (zlib-streams-ts_amd/csrc/zs_bgzf.h: a start sized from its
// header where that can be trusted, by zs_members_size where not) on the CPU, one lane at a time, from
// its own source, with the host stand-ins for the HIP names of tools/lane_host; around it the scan's
// candidate rule (zs_members.h), the plan (zs_plan_members, with its tail rounds) and the planned
// members' trusted flags (zs_plan_bgzf_trusted), as the _bgzf entries run them.  Test tooling: lets the
// CPU suite check the path without a GPU, and a build with -fsanitize=address,undefined shows that no
// lane leaves the aligned words that hold its stream: every stream lies in a buffer of exactly those words.
//
// usage: bgzf_host PASS MODE < streams > results
//   stdin:  u32 count, then per stream: u32 in_len, u32 out_cap, in_len bytes
//   MODE 0: per stream  u32 C, C x u32 candidates, (1 + C) x {how, end, len, reach, trusted} (offset 0's
//           lane, then one per candidate, each bounded by candidate j + PASS + 1), u32 tail rounds, u32
//           in_place, u32 P, P x {in_pos, in_len, out_pos, cap, trusted} (the members zs_plan_members emits
//           and their flags), u32 out_len_ok, u64 out_len (zs_bgzf_chain over the stream)
//   MODE 1: per stream  in_len x {how, end, len, reach, trusted}: a lane from EVERY byte offset, bounded by
//           the stream's end
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hip/hip_runtime.h"
zs_dim3 threadIdx, blockIdx, blockDim;
#include "../../zlib-streams-ts_amd/csrc/zs_bgzf.h"
#define ZS_TOOL "bgzf_host"
#include "host_stream.h"
static void wr_rec(const zs_sync_rec& r, bool trusted) {
  const uint32_t t = trusted;
  wr(&r, 16);
  wr(&t, 4);
}

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
    const HostStream hs(i, n, {0x1f, 0x8b, 0x08, 0x04});  // (bytes that would show as a candidate, or a header)
    const uint8_t* s = hs.s;
    if (mode == 1) {
      for (uint32_t at = 0; at < n; at++) {
        bool t;
        const zs_sync_rec r = zs_bgzf_size(s, n, at, n, T, t);
        if ((r.how != ZS_SYNC_FINAL && r.how != ZS_SYNC_ERROR) || r.end > n) {
          fprintf(stderr, "bgzf_host: stream %u offset %u: an unbounded lane ended in no known way\n", i, at);
          return 3;
        }
        wr_rec(r, t);
      }
    } else {
      const std::vector<uint32_t> cand = host_scan(s, n, [&](uint64_t u, int64_t& q0) { return zs_members_unit(s, n, u, q0); });
      const uint32_t C = (uint32_t)cand.size();
      std::vector<zs_sync_rec> rec(1 + C);
      const uint64_t cfirst[2] = {0, C};
      std::vector<uint8_t> rtrusted(1 + C);
      for (uint32_t x = 0; x <= C; x++) {
        bool at0;
        const uint32_t bound = host_lane(x, cand, pass, n, at0);
        bool t;
        rec[x] = zs_bgzf_size(s, n, at0 ? 0u : cand[x - 1], bound, T, t);
        rtrusted[x] = t;
        if (rec[x].end > (t ? n : bound)) {  // (a trusted lane reads its trailer's word, wherever its bound is)
          fprintf(stderr, "bgzf_host: stream %u lane %u ended at %u, past its bound %u\n", i, x, rec[x].end, bound);
          return 3;
        }
      }
      wr(&C, 4);
      wr(cand.data(), 4ull * C);
      for (uint32_t x = 0; x <= C; x++) wr_rec(rec[x], rtrusted[x]);
      zs_members_plan p;
      uint32_t rounds = 0;
      for (;; rounds++) {  // the tail rounds, as members_batch runs them: members_size's lanes, unbounded
        zs_plan_members(1, &n, &out_cap, cfirst, cand.data(), rec.data(), p);
        if (p.tstream.empty()) break;
        if (rounds > C) {
          fprintf(stderr, "bgzf_host: stream %u: the tail rounds do not end\n", i);
          return 3;
        }
        for (size_t k = 0; k < p.tstream.size(); k++) {
          if (rtrusted[p.trec[k]]) {
            fprintf(stderr, "bgzf_host: stream %u: a trusted record on the tail list\n", i);
            return 3;
          }
          rec[p.trec[k]] = zs_members_size(s, n, p.tstart[k], n, T);
        }
      }
      std::vector<uint8_t> trusted;
      const uint32_t flagged = zs_plan_bgzf_trusted(p, &out_cap, cfirst, cand.data(), rec.data(), rtrusted.data(), trusted);
      const uint32_t P = p.M, inp = p.in_place;
      wr(&rounds, 4);
      wr(&inp, 4);
      wr(&P, 4);
      uint32_t seen = 0;
      for (uint32_t k = 0; k < P; k++) {
        const uint32_t t = trusted[k];
        seen += t;
        wr(&p.soff[k], 4);
        wr(&p.slen[k], 4);
        wr(&p.opos[k], 4);
        wr(&p.ocap[k], 4);
        wr(&t, 4);
      }
      if (seen != flagged) return 3;
      uint64_t total = 0;
      const uint32_t ok = (uint32_t)zs_bgzf_chain(s, n, total);
      if (!ok) total = 0;  // (as zs_bgzf_out_len answers)
      wr(&ok, 4);
      wr(&total, 8);
    }
  }
  return 0;
}
