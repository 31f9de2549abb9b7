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
#if defined(__SANITIZE_ADDRESS__)
#define ZS_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define ZS_ASAN 1
#endif
#endif
#ifdef ZS_ASAN
#include <sanitizer/asan_interface.h>
#endif

static void rd(void* p, size_t n) {
  if (fread(p, 1, n, stdin) != n) {
    fprintf(stderr, "bgzf_host: short input\n");
    exit(2);
  }
}
static void wr(const void* p, size_t n) { fwrite(p, 1, n, stdout); }
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
    // the stream starts `mis` bytes into a 16-byte aligned buffer that ends with the aligned word of its
    // last byte; the whole words in front of its first byte are poisoned (a sanitizer build), so any
    // load outside the aligned words that hold the stream's bytes is reported
    const uint32_t mis = (i * 7u + 1u) % 16u;
    const size_t bytes = ((size_t)mis + n + 3) & ~size_t(3);
    void* raw = nullptr;
    if (posix_memalign(&raw, 16, bytes ? bytes : 4)) return 2;
    uint8_t* buf = (uint8_t*)raw;
    // (a BGZF header's first bytes right around the stream would show if a lane looked there)
    for (size_t k = 0; k < bytes; k++) buf[k] = (const uint8_t[]){0x1f, 0x8b, 0x08, 0x04}[k & 3u];
    uint8_t* s = buf + mis;
    rd(s, n);
#ifdef ZS_ASAN
    if (mis & ~3u) ASAN_POISON_MEMORY_REGION(buf, mis & ~3u);
#endif
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
      std::vector<uint32_t> cand;
      const uint32_t sh16 = (uint32_t)((uintptr_t)s & 15u);
      for (uint64_t u = 0; n && 16u * u < (uint64_t)sh16 + n; u++) {
        int64_t q0;
        uint32_t mask = zs_members_unit(s, n, u, q0);
        for (uint32_t b = 0; b < 16u; b++)
          if (mask >> b & 1u) cand.push_back((uint32_t)(q0 + b));
      }
      const uint32_t C = (uint32_t)cand.size();
      std::vector<zs_sync_rec> rec(1 + C);
      std::vector<uint8_t> rtrusted(1 + C);
      for (uint32_t x = 0; x <= C; x++) {
        const uint64_t bi = (uint64_t)x + pass;  // lane x - 1 of the candidates: j + pass + 1
        const uint32_t bound = bi < C ? cand[bi] : n;
        bool t;
        rec[x] = zs_bgzf_size(s, n, x ? cand[x - 1] : 0u, bound, T, t);
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
      const uint64_t cfirst[2] = {0, C};
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
#ifdef ZS_ASAN
    if (mis & ~3u) ASAN_UNPOISON_MEMORY_REGION(buf, mis & ~3u);
#endif
    free(raw);
  }
  return 0;
}
