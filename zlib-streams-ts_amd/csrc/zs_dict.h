// zs_dict.h -- host-side layout of a batch's preset dictionaries (the
// zs_inflate_batch_dict* entries, capi.cpp / pool.cpp).  Pure functions of the
// caller's (offset, length) arrays: no HIP types, no HIP calls, so the host check
// compiles them with a plain C++ compiler (tools/emu/emu_plan_dict.cpp).
#ifndef ZS_DICT_H
#define ZS_DICT_H
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

// The distinct dictionaries of a batch.  Members may share one (equal offset and
// length): its adler32 is computed once, its bytes are staged once.
struct zs_dict_set {
  std::vector<uint32_t> id;    // per member: its dictionary in uoff / ulen (0 for a member without one)
  std::vector<uint64_t> uoff;  // per distinct dictionary: the caller's offset ...
  std::vector<uint32_t> ulen;  // ... and length (never 0, but for the lone entry of a batch without any)
  bool any = false;            // some member has a dictionary
};

static inline void zs_dict_distinct(uint32_t n, const uint64_t* off, const uint32_t* len, zs_dict_set& d) {
  d.id.assign(n, 0);
  d.uoff.clear();
  d.ulen.clear();
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < n; i++)
    if (len[i]) order.push_back(i);
  d.any = !order.empty();
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return off[a] != off[b] ? off[a] < off[b] : len[a] != len[b] ? len[a] < len[b] : a < b;
  });
  for (size_t k = 0; k < order.size(); k++) {
    const uint32_t i = order[k];
    if (k == 0 || off[i] != d.uoff.back() || len[i] != d.ulen.back()) {
      d.uoff.push_back(off[i]);
      d.ulen.push_back(len[i]);
    }
    d.id[i] = (uint32_t)d.uoff.size() - 1;
  }
  if (d.uoff.empty()) {  // (the arrays are never empty: id 0 always names an entry)
    d.uoff.push_back(0);
    d.ulen.push_back(0);
  }
}

// The host entries' staging: the distinct dictionaries back to back (any byte
// alignment: the kernels read aligned words around them).  poff[i]: member i's
// offset in the staging (0 without a dictionary); returns its size.
static inline uint64_t zs_dict_pack_layout(const zs_dict_set& d, uint32_t n, const uint32_t* len,
                                           std::vector<uint64_t>& upos, std::vector<uint64_t>& poff) {
  upos.resize(d.uoff.size());
  uint64_t total = 0;
  for (size_t k = 0; k < d.uoff.size(); k++) {
    upos[k] = total;
    total += d.ulen[k];
  }
  poff.assign(n, 0);
  for (uint32_t i = 0; i < n; i++)
    if (len[i]) poff[i] = upos[d.id[i]];
  return total;
}
static inline void zs_dict_pack(const zs_dict_set& d, const std::vector<uint64_t>& upos, const uint8_t* dict,
                                uint8_t* dst) {
  for (size_t k = 0; k < d.uoff.size(); k++)
    if (d.ulen[k]) memcpy(dst + upos[k], dict + d.uoff[k], d.ulen[k]);
}

#endif
