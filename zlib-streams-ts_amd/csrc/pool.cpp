// pool.cpp -- host-side entry points above the per-device context
// (include/zs_gpu.h): unbounded-output decode and the multi-GPU pool.
//
// * zs_inflate_batch_auto: DecompressionStream semantics for the output size.
//   The reference's stream layer loops over pooled 64 KiB output buffers until
//   Z_STREAM_END (src/mod/streams.ts:46,132-182), so a member's output is never
//   capped.  Here a first pass decodes every member into a capacity guessed
//   from its input; the members that ran out of room (ZS_MSG_CAPACITY, a
//   condition the reference cannot have) are decoded again, only they, with
//   eight times the room, until every member fits.  Decoding is deterministic
//   and the capacity only decides whether a member fits, so the bytes, status
//   and message of every member are those of an unbounded decode.
// * zs_pool_*: one context per device of a device mask; a batch is split into
//   contiguous stream ranges shard_range(n, G, k) = [k n / G, (k + 1) n / G)
//   (SURVEY.md 8(e)), one host thread per device, each writing its streams'
//   results straight into the caller's arrays at their own offsets.  No data
//   crosses devices: the host already holds every stream's size, so the only
//   collective of the multi-process path (the RCCL size all-gather,
//   zsamd/shard.py) is not needed inside one process.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zs_gpu.h"
#include "zs_inflate.h"
#include "zs_plan.h"  // zs_wbits_split

void zs_set_last_error(const std::string& msg);  // capi.cpp: what zs_last_error() returns on this thread

namespace {

struct Shard {
  uint32_t a, b;
};

Shard shard_range(uint32_t n, uint32_t g, uint32_t k) {
  return {(uint32_t)((uint64_t)n * k / g), (uint32_t)((uint64_t)n * (k + 1) / g)};
}

constexpr uint64_t kCapMax = 0xfffffffcull;  // largest u32 capacity that is a multiple of 4

uint32_t first_cap(uint32_t in_len) {
  const uint64_t c = std::max<uint64_t>(65536, 4ull * in_len);
  return (uint32_t)std::min<uint64_t>(kCapMax, (c + 3) & ~3ull);
}

}  // namespace

extern "C" void zs_free(void* p) { free(p); }

// One bounded batch of the unbounded decode: with dictionaries when dict_off is given
static int inflate_bounded(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                           const uint32_t* in_len, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                           int32_t* status, int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed,
                           uint32_t* check, const uint8_t* dict, const uint64_t* dict_off, const uint32_t* dict_len) {
  if (dict_off)
    return zs_inflate_batch_dict(c, wbits, n, in, in_off, in_len, out, out_off, out_cap, status, phase, msg, out_len,
                                 consumed, check, dict, dict_off, dict_len);
  return zs_inflate_batch_ex(c, wbits, n, in, in_off, in_len, out, out_off, out_cap, status, phase, msg, out_len,
                             consumed, check);
}

// zs_inflate_batch_auto, and zs_inflate_batch_dict_auto when dict_off is given
static int inflate_auto(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                        const uint32_t* in_len, uint8_t** out, uint64_t* out_off, int32_t* status, int32_t* phase,
                        int32_t* msg, uint32_t* out_len, uint32_t* consumed, uint32_t* check, const uint8_t* dict,
                        const uint64_t* dict_off, const uint32_t* dict_len) {
  if (!out || !out_off) return ZS_STREAM_ERROR;
  *out = nullptr;
  // pass buffers: pass 0 holds every member, later passes the retried ones
  // (buffers uninitialised: the host entry writes only the produced bytes, so
  // pages of capacity a member does not use are never touched)
  struct Pass {
    std::vector<uint32_t> idx, cap;
    std::vector<uint64_t> off;
    std::unique_ptr<uint8_t, decltype(&free)> buf{nullptr, &free};
    bool alloc(uint64_t bytes) {
      buf.reset((uint8_t*)malloc(bytes));
      return buf != nullptr;
    }
  };
  std::vector<Pass> passes(1);
  std::vector<uint32_t> where(n, 0);   // the pass a member's final output is in
  std::vector<uint32_t> slot(n, 0);    // its index in that pass
  {
    Pass& p = passes[0];
    p.idx.resize(n);
    p.cap.resize(n);
    p.off.resize(n);
    uint64_t o = 0;
    for (uint32_t i = 0; i < n; i++) {
      p.idx[i] = i;
      p.cap[i] = first_cap(in_len[i]);
      p.off[i] = o;
      o += p.cap[i];
      slot[i] = i;
    }
    if (!p.alloc(o + 4)) return ZS_MEM_ERROR;
    const int r = inflate_bounded(c, wbits, n, in, in_off, in_len, p.buf.get(), p.off.data(), p.cap.data(), status,
                                  phase, msg, out_len, consumed, check, dict, dict_off, dict_len);
    if (r != ZS_OK) return r;
  }
  for (;;) {
    const Pass& last = passes.back();
    Pass nx;
    uint64_t o = 0;
    for (size_t k = 0; k < last.idx.size(); k++) {
      const uint32_t i = last.idx[k];
      if (!(status[i] == ZS_BUF_ERROR && msg[i] == ZS_MSG_CAPACITY) || last.cap[k] >= kCapMax) continue;
      nx.idx.push_back(i);
      const uint32_t cap = (uint32_t)std::min<uint64_t>(kCapMax, 8ull * last.cap[k]);
      nx.cap.push_back(cap);
      nx.off.push_back(o);
      o += cap;
    }
    if (nx.idx.empty()) break;
    const uint32_t m = (uint32_t)nx.idx.size();
    std::vector<uint64_t> ioff(m), doff(dict_off ? m : 0);
    std::vector<uint32_t> ilen(m), cons(m), olen(m), chk(m), dlen(dict_off ? m : 0);
    std::vector<int32_t> st(m), ph(m), ms(m);
    for (uint32_t k = 0; k < m; k++) {
      ioff[k] = in_off[nx.idx[k]];
      ilen[k] = in_len[nx.idx[k]];
      if (dict_off) {
        doff[k] = dict_off[nx.idx[k]];
        dlen[k] = dict_len[nx.idx[k]];
      }
    }
    if (!nx.alloc(o + 4)) return ZS_MEM_ERROR;
    const int r = inflate_bounded(c, wbits, m, in, ioff.data(), ilen.data(), nx.buf.get(), nx.off.data(),
                                  nx.cap.data(), st.data(), ph.data(), ms.data(), olen.data(), cons.data(),
                                  check ? chk.data() : nullptr, dict, dict_off ? doff.data() : nullptr, dlen.data());
    if (r != ZS_OK) return r;
    for (uint32_t k = 0; k < m; k++) {
      const uint32_t i = nx.idx[k];
      status[i] = st[k];
      phase[i] = ph[k];
      msg[i] = ms[k];
      out_len[i] = olen[k];
      consumed[i] = cons[k];
      if (check) check[i] = chk[k];
      where[i] = (uint32_t)passes.size();
      slot[i] = k;
    }
    passes.push_back(std::move(nx));
  }
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    out_off[i] = total;
    total += out_len[i];
  }
  uint8_t* res = (uint8_t*)malloc(total ? total : 1);
  if (!res) return ZS_MEM_ERROR;
  for (uint32_t i = 0; i < n; i++)
    if (out_len[i]) {
      const Pass& p = passes[where[i]];
      memcpy(res + out_off[i], p.buf.get() + p.off[slot[i]], out_len[i]);
    }
  *out = res;
  return ZS_OK;
}

extern "C" int zs_inflate_batch_auto(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                     const uint32_t* in_len, uint8_t** out, uint64_t* out_off, int32_t* status,
                                     int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed,
                                     uint32_t* check) {
  return inflate_auto(c, wbits, n, in, in_off, in_len, out, out_off, status, phase, msg, out_len, consumed, check,
                      nullptr, nullptr, nullptr);
}

// with preset dictionaries (inflateSetDictionary, inflate.ts:1220-1249; Z_NEED_DICT, inflate.ts:594-597)
extern "C" int zs_inflate_batch_dict_auto(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in,
                                          const uint64_t* in_off, const uint32_t* in_len, uint8_t** out,
                                          uint64_t* out_off, int32_t* status, int32_t* phase, int32_t* msg,
                                          uint32_t* out_len, uint32_t* consumed, uint32_t* check, const uint8_t* dict,
                                          const uint64_t* dict_off, const uint32_t* dict_len) {
  if (!dict_off || !dict_len) {
    zs_set_last_error("null dictionary arrays");
    return ZS_STREAM_ERROR;
  }
  return inflate_auto(c, wbits, n, in, in_off, in_len, out, out_off, status, phase, msg, out_len, consumed, check,
                      dict, dict_off, dict_len);
}

// ------------------------------------------------------------------ pool
struct zs_pool {
  std::vector<int> devices;
  std::vector<zs_ctx*> ctx;
  std::mutex mtx;  // one batch at a time (the contexts' workspaces are reused)
};

extern "C" int zs_pool_create(uint64_t device_mask, zs_pool** out) {
  if (!out) return ZS_STREAM_ERROR;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    zs_set_last_error("no HIP device");
    return ZS_STREAM_ERROR;
  }
  zs_pool* p = new zs_pool();
  for (int d = 0; d < std::min(ndev, 64); d++)
    if (device_mask == 0 || ((device_mask >> d) & 1u)) p->devices.push_back(d);
  const uint64_t known = ndev >= 64 ? ~0ull : (1ull << ndev) - 1;
  if (p->devices.empty() || (device_mask & ~known) != 0) {
    delete p;
    zs_set_last_error("device mask names no device, or a device that does not exist");
    return ZS_STREAM_ERROR;
  }
  for (int d : p->devices) {
    zs_ctx* c = nullptr;
    const int r = zs_ctx_create(d, &c);
    if (r != ZS_OK) {
      const std::string e = zs_last_error();
      zs_pool_destroy(p);
      zs_set_last_error(e);
      return r;
    }
    p->ctx.push_back(c);
  }
  *out = p;
  return ZS_OK;
}

extern "C" int zs_pool_create_list(const int* devices, int n, zs_pool** out) {
  if (!out || !devices || n <= 0) {
    zs_set_last_error("invalid arguments");
    return ZS_STREAM_ERROR;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    zs_set_last_error("no HIP device");
    return ZS_STREAM_ERROR;
  }
  zs_pool* p = new zs_pool();
  for (int k = 0; k < n; k++) {
    if (devices[k] < 0 || devices[k] >= ndev) {
      delete p;
      zs_set_last_error("device list names a device that does not exist");
      return ZS_STREAM_ERROR;
    }
    p->devices.push_back(devices[k]);
  }
  for (int d : p->devices) {
    zs_ctx* c = nullptr;
    const int r = zs_ctx_create(d, &c);
    if (r != ZS_OK) {
      const std::string e = zs_last_error();
      zs_pool_destroy(p);
      zs_set_last_error(e);
      return r;
    }
    p->ctx.push_back(c);
  }
  *out = p;
  return ZS_OK;
}

extern "C" void zs_pool_destroy(zs_pool* p) {
  if (!p) return;
  for (zs_ctx* c : p->ctx) zs_ctx_destroy(c);
  delete p;
}

extern "C" int zs_pool_size(const zs_pool* p) { return p ? (int)p->devices.size() : 0; }
extern "C" int zs_pool_device(const zs_pool* p, int k) {
  return p && k >= 0 && k < (int)p->devices.size() ? p->devices[k] : -1;
}

// Runs fn(k, shard) for every device k on its own thread; returns the first
// failing code (its message in zs_last_error() on the calling thread).
template <class F>
static int run_sharded(zs_pool* p, uint32_t n, F fn) {
  if (!p) {
    zs_set_last_error("null pool");
    return ZS_STREAM_ERROR;
  }
  std::lock_guard<std::mutex> lk(p->mtx);
  const uint32_t G = (uint32_t)p->ctx.size();
  std::vector<int> rc(G, ZS_OK);
  std::vector<std::string> err(G);
  std::vector<std::thread> th;
  for (uint32_t k = 0; k < G; k++)
    th.emplace_back([&, k] {
      const Shard s = shard_range(n, G, k);
      rc[k] = fn(k, s);
      if (rc[k] != ZS_OK) err[k] = zs_last_error();
    });
  for (auto& t : th) t.join();
  for (uint32_t k = 0; k < G; k++)
    if (rc[k] != ZS_OK) {
      zs_set_last_error("device " + std::to_string(p->devices[k]) + ": " + err[k]);
      return rc[k];
    }
  return ZS_OK;
}

extern "C" int zs_pool_deflate_batch(zs_pool* p, int level, int wbits, uint32_t n, const uint8_t* in,
                                     const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                     const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                     uint32_t* out_len, uint32_t* check) {
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_deflate_batch_ex(p->ctx[k], level, wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out,
                               out_off + s.a, out_cap + s.a, status + s.a, out_len + s.a,
                               check ? check + s.a : nullptr);
  });
}

// with a compression strategy (deflate.ts:289-290, :923-931)
extern "C" int zs_pool_deflate_batch_strategy(zs_pool* p, int level, int strategy, int wbits, uint32_t n,
                                              const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                              uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                              int32_t* status, uint32_t* out_len, uint32_t* check) {
  if (strategy < 0 || strategy > ZS_FIXED) {
    zs_set_last_error("invalid strategy");
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_deflate_batch_strategy(p->ctx[k], level, strategy, wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out,
                                     out_off + s.a, out_cap + s.a, status + s.a, out_len + s.a,
                                     check ? check + s.a : nullptr);
  });
}

// with deflateInit2_'s windowBits and memLevel (deflate.ts:253-343; validation :281-294)
extern "C" int zs_pool_deflate_batch_params(zs_pool* p, int level, int wbits, int mem_level, uint32_t n,
                                            const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                            uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                            int32_t* status, uint32_t* out_len, uint32_t* check) {
  int wrap;
  if (!zs_wbits_split(wbits, &wrap)) {
    zs_set_last_error("invalid window bits");
    return ZS_STREAM_ERROR;
  }
  if (mem_level < 1 || mem_level > 9) {
    zs_set_last_error("invalid memLevel");
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_deflate_batch_params(p->ctx[k], level, wbits, mem_level, s.b - s.a, in, in_off + s.a, in_len + s.a, out,
                                   out_off + s.a, out_cap + s.a, status + s.a, out_len + s.a,
                                   check ? check + s.a : nullptr);
  });
}

// with preset dictionaries (deflateSetDictionary, deflate.ts:367-424; FDICT / DICTID, deflate.ts:767-778):
// every shard reads the caller's one dictionary buffer
extern "C" int zs_pool_deflate_batch_dict(zs_pool* p, int level, int wbits, uint32_t n, const uint8_t* in,
                                          const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                          const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                          uint32_t* out_len, uint32_t* check, const uint8_t* dict,
                                          const uint64_t* dict_off, const uint32_t* dict_len) {
  if (!dict_off || !dict_len) {
    zs_set_last_error("null dictionary arrays");
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_deflate_batch_dict(p->ctx[k], level, wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out,
                                 out_off + s.a, out_cap + s.a, status + s.a, out_len + s.a,
                                 check ? check + s.a : nullptr, dict, dict_off + s.a, dict_len + s.a);
  });
}

// BGZF: sharded by stream; the faults of the level, the block size and the arrays first, as the
// context's entries name them
extern "C" int zs_pool_deflate_batch_bgzf(zs_pool* p, int level, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                          const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                          const uint32_t* out_cap, int32_t* status, uint32_t* out_len, uint32_t* check,
                                          uint32_t block_bytes) {
  const char* msg = level < -1 || level > 9                               ? "invalid level"
                    : block_bytes > ZS_BGZF_BLOCK                         ? "invalid BGZF block size"
                    : n && (!in_off || !in_len || !out_off || !out_cap)   ? "null arrays"
                                                                          : nullptr;
  if (msg) {
    zs_set_last_error(msg);
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_deflate_batch_bgzf(p->ctx[k], level, s.b - s.a, in, in_off + s.a, in_len + s.a, out, out_off + s.a,
                                 out_cap + s.a, status + s.a, out_len + s.a, check ? check + s.a : nullptr,
                                 block_bytes);
  });
}

// with Z_FULL_FLUSH points (deflate.ts:942-961): sharded by stream, every shard reads the caller's one
// position array through its part of the index
extern "C" int zs_pool_deflate_batch_flush(zs_pool* p, int level, int wbits, uint32_t n, const uint8_t* in,
                                           const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                           const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                           uint32_t* out_len, uint32_t* check, int flush, const uint64_t* flush_first,
                                           const uint32_t* flush_pos) {
  if (flush != ZS_FULL_FLUSH) {
    zs_set_last_error(flush == 1 || flush == 2 || flush == 5 ? "flush mode not built" : "invalid flush");
    return ZS_STREAM_ERROR;
  }
  if (n && !flush_first) {
    zs_set_last_error("null flush arrays");
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_deflate_batch_flush(p->ctx[k], level, wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out,
                                  out_off + s.a, out_cap + s.a, status + s.a, out_len + s.a,
                                  check ? check + s.a : nullptr, flush, flush_first + s.a, flush_pos);
  });
}

// the restart points found from the bytes (inflate.ts:1267-1337): sharded by stream, every shard finds its own
extern "C" int zs_pool_inflate_batch_sync(zs_pool* p, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                          const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                          const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                          uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  zs_inflate_call a;
  a.n = n;
  a.out_cap = out_cap;
  if (const zs_sync_err e = zs_sync_validate(wbits, a)) {
    zs_set_last_error(zs_sync_err_text(e));
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_inflate_batch_sync(p->ctx[k], wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out, out_off + s.a,
                                 out_cap + s.a, status + s.a, phase + s.a, msg + s.a, out_len + s.a, consumed + s.a,
                                 check ? check + s.a : nullptr);
  });
}

// every member of multi-member gzip files (zlib's gz_look, gzread.c): sharded by stream, the members stay
// inside their stream
extern "C" int zs_pool_inflate_batch_members(zs_pool* p, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                             const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                             const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                             uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  zs_inflate_call a;
  a.n = n;
  a.out_cap = out_cap;
  if (const zs_members_err e = zs_members_validate(wbits, a)) {
    zs_set_last_error(zs_members_err_text(e));
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_inflate_batch_members(p->ctx[k], wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out, out_off + s.a,
                                    out_cap + s.a, status + s.a, phase + s.a, msg + s.a, out_len + s.a, consumed + s.a,
                                    check ? check + s.a : nullptr);
  });
}

// BGZF files, the members sized from their headers where those can be trusted: sharded as the
// members entry
extern "C" int zs_pool_inflate_batch_bgzf(zs_pool* p, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                          const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                          const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                          uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  zs_inflate_call a;
  a.n = n;
  a.out_cap = out_cap;
  if (const zs_members_err e = zs_members_validate(wbits, a)) {
    zs_set_last_error(zs_members_err_text(e));
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_inflate_batch_bgzf(p->ctx[k], wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out, out_off + s.a,
                                 out_cap + s.a, status + s.a, phase + s.a, msg + s.a, out_len + s.a, consumed + s.a,
                                 check ? check + s.a : nullptr);
  });
}

// BGZF ranges by virtual offset: sharded by stream as the _bgzf entry, the refusals first
extern "C" int zs_pool_inflate_batch_bgzf_range(zs_pool* p, int wbits, uint32_t n, const uint8_t* in,
                                                const uint64_t* in_off, const uint32_t* in_len,
                                                const uint64_t* voff_begin, const uint64_t* voff_end, uint8_t* out,
                                                const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                                int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed,
                                                uint32_t* check) {
  zs_inflate_call a;
  a.n = n;
  a.out_cap = out_cap;
  if (const zs_members_err e = zs_members_validate(wbits, a)) {
    zs_set_last_error(zs_members_err_text(e));
    return ZS_STREAM_ERROR;
  }
  if (const zs_bgzf_range_err e = zs_bgzf_range_validate(n, in_len, voff_begin, voff_end)) {
    zs_set_last_error(zs_bgzf_range_err_text(e));
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_inflate_batch_bgzf_range(p->ctx[k], wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, voff_begin + s.a,
                                       voff_end + s.a, out, out_off + s.a, out_cap + s.a, status + s.a, phase + s.a,
                                       msg + s.a, out_len + s.a, consumed + s.a, check ? check + s.a : nullptr);
  });
}

// from restart points (inflate.ts:1267-1337): sharded by stream, every shard reads the caller's point arrays
// through its part of the index
extern "C" int zs_pool_inflate_batch_restart(zs_pool* p, int wbits, uint32_t n, const uint8_t* in,
                                             const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                             const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                             int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed,
                                             uint32_t* check, const uint64_t* restart_first,
                                             const uint32_t* restart_in, const uint32_t* restart_out) {
  zs_restart_call a;
  a.n = n;
  a.in_len = in_len;
  a.out_cap = out_cap;
  a.rfirst = restart_first;
  a.rin = restart_in;
  a.rout = restart_out;
  if (const zs_restart_err e = zs_restart_validate(wbits, a)) {
    zs_set_last_error(zs_restart_err_text(e));
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_inflate_batch_restart(p->ctx[k], wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out, out_off + s.a,
                                    out_cap + s.a, status + s.a, phase + s.a, msg + s.a, out_len + s.a,
                                    consumed + s.a, check ? check + s.a : nullptr, restart_first + s.a, restart_in,
                                    restart_out);
  });
}

// with primed pieces: sharded by stream as the flushed form
extern "C" int zs_pool_deflate_batch_primed(zs_pool* p, int level, int wbits, uint32_t n, const uint8_t* in,
                                            const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                            const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                            uint32_t* out_len, uint32_t* check, const uint64_t* flush_first,
                                            const uint32_t* flush_pos) {
  if (n && !flush_first) {
    zs_set_last_error("null flush arrays");
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_deflate_batch_primed(p->ctx[k], level, wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out,
                                   out_off + s.a, out_cap + s.a, status + s.a, out_len + s.a,
                                   check ? check + s.a : nullptr, flush_first + s.a, flush_pos);
  });
}

extern "C" int zs_pool_inflate_batch(zs_pool* p, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                     const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                     const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                     uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_inflate_batch_ex(p->ctx[k], wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out, out_off + s.a,
                               out_cap + s.a, status + s.a, phase + s.a, msg + s.a, out_len + s.a,
                               consumed + s.a, check ? check + s.a : nullptr);
  });
}

// zs_pool_inflate_batch_auto, and zs_pool_inflate_batch_dict_auto when dict_off is given
static int pool_inflate_auto(zs_pool* p, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                             const uint32_t* in_len, uint8_t** out, uint64_t* out_off, int32_t* status,
                             int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed, uint32_t* check,
                             const uint8_t* dict, const uint64_t* dict_off, const uint32_t* dict_len) {
  if (!out || !out_off) return ZS_STREAM_ERROR;
  *out = nullptr;
  const uint32_t G = p ? (uint32_t)p->ctx.size() : 0;
  std::vector<uint8_t*> part(G, nullptr);
  const int r = run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return inflate_auto(p->ctx[k], wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, &part[k], out_off + s.a,
                        status + s.a, phase + s.a, msg + s.a, out_len + s.a, consumed + s.a,
                        check ? check + s.a : nullptr, dict, dict_off ? dict_off + s.a : nullptr,
                        dict_off ? dict_len + s.a : nullptr);
  });
  if (r == ZS_OK) {  // one buffer: the shards' outputs back to back, offsets rebased
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += out_len[i];
    uint8_t* res = (uint8_t*)malloc(total ? total : 1);
    if (res) {
      uint64_t base = 0;
      for (uint32_t k = 0; k < G; k++) {
        const Shard s = shard_range(n, G, k);
        uint64_t bytes = 0;
        for (uint32_t i = s.a; i < s.b; i++) bytes += out_len[i];
        if (bytes) memcpy(res + base, part[k], bytes);
        for (uint32_t i = s.a; i < s.b; i++) out_off[i] += base;
        base += bytes;
      }
      *out = res;
    }
    for (uint8_t* q : part) free(q);
    return res ? ZS_OK : ZS_MEM_ERROR;
  }
  for (uint8_t* q : part) free(q);
  return r;
}

extern "C" int zs_pool_inflate_batch_auto(zs_pool* p, int wbits, uint32_t n, const uint8_t* in,
                                          const uint64_t* in_off, const uint32_t* in_len, uint8_t** out,
                                          uint64_t* out_off, int32_t* status, int32_t* phase, int32_t* msg,
                                          uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  return pool_inflate_auto(p, wbits, n, in, in_off, in_len, out, out_off, status, phase, msg, out_len, consumed, check,
                           nullptr, nullptr, nullptr);
}

// The pool entries with preset dictionaries (inflateSetDictionary, inflate.ts:1220-1249; Z_NEED_DICT,
// inflate.ts:594-597): every shard reads the caller's one dictionary buffer
extern "C" int zs_pool_inflate_batch_dict(zs_pool* p, int wbits, uint32_t n, const uint8_t* in,
                                          const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                          const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                          int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed,
                                          uint32_t* check, const uint8_t* dict, const uint64_t* dict_off,
                                          const uint32_t* dict_len) {
  if (!dict_off || !dict_len) {
    zs_set_last_error("null dictionary arrays");
    return ZS_STREAM_ERROR;
  }
  return run_sharded(p, n, [&](uint32_t k, Shard s) {
    if (s.a == s.b) return (int)ZS_OK;
    return zs_inflate_batch_dict(p->ctx[k], wbits, s.b - s.a, in, in_off + s.a, in_len + s.a, out, out_off + s.a,
                                 out_cap + s.a, status + s.a, phase + s.a, msg + s.a, out_len + s.a,
                                 consumed + s.a, check ? check + s.a : nullptr, dict, dict_off + s.a,
                                 dict_len + s.a);
  });
}

extern "C" int zs_pool_inflate_batch_dict_auto(zs_pool* p, int wbits, uint32_t n, const uint8_t* in,
                                               const uint64_t* in_off, const uint32_t* in_len, uint8_t** out,
                                               uint64_t* out_off, int32_t* status, int32_t* phase, int32_t* msg,
                                               uint32_t* out_len, uint32_t* consumed, uint32_t* check,
                                               const uint8_t* dict, const uint64_t* dict_off,
                                               const uint32_t* dict_len) {
  if (!dict_off || !dict_len) {
    zs_set_last_error("null dictionary arrays");
    return ZS_STREAM_ERROR;
  }
  return pool_inflate_auto(p, wbits, n, in, in_off, in_len, out, out_off, status, phase, msg, out_len, consumed, check,
                           dict, dict_off, dict_len);
}
