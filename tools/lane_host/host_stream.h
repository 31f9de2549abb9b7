// What tools/sync_host, members_host and bgzf_host share: stdin and stdout, a stream placed so that a
// sanitizer build reports any load outside the aligned words that hold it, the scan over its 16-byte units
// and the sizing lanes' numbering as the kernels have it (zs_cand.h).  Test tooling only.  ZS_TOOL: the
// tool's name in its messages.
#pragma once
#include <stdlib.h>
#include <vector>
#include "../../zlib-streams-ts_amd/csrc/zs_cand.h"
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
    fprintf(stderr, ZS_TOOL ": short input\n");
    exit(2);
  }
}
static void wr(const void* p, size_t n) { fwrite(p, 1, n, stdout); }

// Stream i of the input, n bytes read from stdin: it starts `mis` bytes into a 16-byte aligned buffer that ends
// with the aligned word of its last byte; the whole words in front of its first byte are poisoned (a sanitizer
// build), so any load outside the aligned words that hold the stream's bytes is reported.  fill: four bytes
// repeated around the stream, which would show as a candidate if the scan looked there.
struct HostStream {
  void* raw = nullptr;
  uint8_t* s = nullptr;
  uint32_t mis;
  HostStream(uint32_t i, uint32_t n, const uint8_t (&fill)[4]) : mis((i * 7u + 1u) % 16u) {
    const size_t bytes = ((size_t)mis + n + 3) & ~size_t(3);
    if (posix_memalign(&raw, 16, bytes ? bytes : 4)) exit(2);
    uint8_t* buf = (uint8_t*)raw;
    for (size_t k = 0; k < bytes; k++) buf[k] = fill[k & 3u];
    s = buf + mis;
    rd(s, n);
#ifdef ZS_ASAN
    if (mis & ~3u) ASAN_POISON_MEMORY_REGION(buf, mis & ~3u);
#endif
  }
  ~HostStream() {
#ifdef ZS_ASAN
    if (mis & ~3u) ASAN_UNPOISON_MEMORY_REGION(raw, mis & ~3u);
#endif
    free(raw);
  }
};

// the candidates of a stream: unit(u, q0) is the scan's rule over unit u (zs_sync_unit, zs_members_unit)
template <class Unit>
static std::vector<uint32_t> host_scan(const uint8_t* s, uint32_t n, Unit unit) {
  std::vector<uint32_t> cand;
  const uint32_t sh16 = (uint32_t)((uintptr_t)s & 15u);
  for (uint64_t u = 0; n && 16u * u < (uint64_t)sh16 + n; u++) {
    int64_t q0;
    const uint32_t mask = unit(u, q0);
    for (uint32_t b = 0; b < 16u; b++)
      if (mask >> b & 1u) cand.push_back((uint32_t)(q0 + b));
  }
  return cand;
}
// Lane x of the one stream's sizing launch, as the kernels number and bound it: one stream, one tile, C candidates.
// Returns the lane's bound; first: whether it starts at the stream's first point, else at cand[x - 1].
static uint32_t host_lane(uint32_t x, const std::vector<uint32_t>& cand, uint32_t pass, uint32_t n, bool& first) {
  const uint32_t stile[2] = {0, 1};
  const uint64_t tpre[2] = {0, cand.size()};
  const zs_cand_lane l = zs_cand_lookup(x, 1, stile, tpre);
  first = l.k == ZS_CAND_FIRST;
  if (!first && l.k != x - 1u) exit(3);
  return zs_cand_bound(l, stile, tpre, cand.data(), pass, n);
}
