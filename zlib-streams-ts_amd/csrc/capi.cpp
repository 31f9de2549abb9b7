// capi.cpp -- the C-ABI host layer of libzsgpu.so (include/zs_gpu.h).
//
// Owns one device context per GPU: a HIP stream, a growable device workspace
// and the launch sequence of the batch engines.  No torch types cross this
// boundary; callers hand in plain pointers (device or host) and sizes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zs_gpu.h"
#include "zs_common.h"
#include "zs_kernels.h"
#include "zs_inflate.h"
#include "zs_split.h"
#include "zs_seg.h"
#include "zs_plan.h"
#include "zs_sweep_ring.h"
#include "zs_dict.h"
#define ZS_BGZF_HOST_ONLY 1
#include "zs_bgzf.h"


namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, const char* a = "") {
  char buf[512];
  snprintf(buf, sizeof buf, fmt, a);
  g_err = buf;
  return code;
}

#define HIPCHK(x)                                                          \
  do {                                                                     \
    hipError_t e_ = (x);                                                   \
    if (e_ != hipSuccess) return fail(ZS_MEM_ERROR, "%s", hipGetErrorString(e_)); \
  } while (0)

// Device workspace, or pinned host staging (kHost): grows on demand, is reused
// across calls and freed with its owner (the context's device current).
template <bool kHost>
struct BufT {
  void* p = nullptr;
  size_t cap = 0;
  BufT() = default;
  BufT(const BufT&) = delete;
  BufT& operator=(const BufT&) = delete;
  ~BufT() { release(); }
  void release() {
    if (p) (void)(kHost ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = std::max<size_t>(bytes + bytes / 8, kHost ? 1 << 20 : 4096);
    hipError_t e = kHost ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    else p = nullptr;
    return e;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};
using Buf = BufT<false>;
using HostBuf = BufT<true>;

}  // namespace

void zs_set_last_error(const std::string& msg) { g_err = msg; }

struct zs_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool timing = false;
  bool check_phases = false;  // synchronise after every phase and name the one that failed
  zs_route_opts o;            // the options that decide routes and instances (zs_plan.h)
  // what the current batch's plan decided (zs_plan.h; their vectors are reused across calls)
  zs_deflate_plan dp;
  zs_inflate_plan ip;
  zs_seg_plan gp;
  // workspace
  Buf meta, prevd, mres, syms, blocks, streams, codes, hdr, check, istate, pscr, ltabs, lres, llen, lstat;
  bool fast_group = true;    // L1..3: zs_k_fast (group-speculative) instead of zs_k_fast_serial
  // the chain builders (zs_k_bucket, zs_k_prev, zs_k_fast) let same-address LDS atomics of
  // one instruction apply in lane order (1) or rank equal hashes by ballots (0); 0 when the
  // self-test finds the order violated on this device
  bool lane_order = true;
  bool lane_order_ok = true;  // the self-test's verdict
  hipStream_t side = nullptr;         // second stream: the wave-per-member kernel runs beside the lane kernel
  hipStream_t side2 = nullptr;        // third: the split decode, beside the segmented decode
  hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr;
  Buf wlist;
  Buf dadler, d_dict;  // preset dictionaries: the distinct ones' adler32; the host entries' staging of their bytes
  Buf djoin;           // deflate with dictionaries: the joined streams (zs_k_dict_join)
  Buf ghead;           // levels 1..3 at memLevel 9 and a large window: head[] per stream (zs_plan_fast_params)
  Buf fstreams, fscan;  // a batch with flush points: the streams' records (`streams` holds the segments'); the layout scan
  zs_flush_plan fp;
  // The record of the current public call, which the zs_last_* counters read.  call_begin clears it; the
  // functions that plan and launch a device batch (a host call's chunks, a restart call's segments) only add.
  struct FlushIdx {
    size_t at;  // u64 index of the device call's scan in fscan
    uint32_t n, M, hl;
    std::vector<uint32_t> sfirst;
    // a BGZF device call (zs_last_bgzf_blocks): the segments' input offsets, the streams' lengths, and at
    // level 0, where no scan runs, the members' size
    bool bgzf = false;
    std::vector<uint32_t> soff, in_len;
    uint32_t stored_member = 0;
  };
  struct Call {
    uint32_t ck_parts = 0;     // the data checksum's parts (zs_last_checksum_parts)
    uint32_t host_chunks = 0;  // the chunks of a host-buffer call (zs_last_host_chunks)
    // the flushed device calls of the compress call (a host entry's chunks, one after the other in fscan):
    // where their scans lie and which segments start their streams (zs_last_flush_index)
    std::vector<FlushIdx> fidx;
    size_t fscan_at = 0, fscan_used = 0;  // the current device call's scan in fscan; u64 values in use
    bool seg_ran = false;       // a segmented launch has run: its count of members finished goes on
    bool lanes_zeroed = false;  // the lane counter (lstat) has been zeroed
    bool sync = false;          // the points were found by the call (zs_last_restart_points)
    bool members = false;       // the members were found by the call (zs_last_members)
    uint32_t bgzf_trusted = 0;  // a _bgzf call's planned members sized from their headers (zs_last_bgzf_trusted)
  } call;
  // The entries that decode a stream's pieces as the members of one batch (restart points given, DESIGN 4.11, or
  // found, 4.13; a gzip file's members, 4.14; BGZF blocks, 4.15, and ranges, 4.17).  One public call runs one
  // search and one piece decode, so each has one family of buffers.
  // The search (cand_search, cand_tail): the streams' arrays, first points and tiles; the scan's tiles; the
  // candidates; the lanes' records and, in a _bgzf call, a byte per record; the tail rounds' lists and records
  Buf fmeta, ftile, fcand, frec, ftail, ftrust;
  // The pieces (pieces_begin, pieces_decode): a members or range call's arrays for the place and the stitch, the
  // pieces' results (5 arrays of M), the staging route's regions, the lengths the check values are taken over
  Buf pseg, pres, pstage, plen;
  std::vector<uint8_t> hsec, hck;  // the host's copy of the section being uploaded; of a check value's part map
  // a restart call's own: the closed copies of the segments, their marker flags, the streams' checksums and
  // trailer values (2 arrays of n)
  Buf rgather, rmark, rsum;
  zs_restart_plan rp;
  zs_sync_plan yp;         // the found points, which zs_last_restart_points returns
  zs_members_plan mp;      // the found members, which zs_last_members returns
  zs_bgzf_range_plan brp;  // a _bgzf_range call's plan
  zs_dict_set dset;
  zs_checksum_plan cp;     // the current batch's data checksum (zs_plan_checksum)
  Buf ckvals;              // ... its parts' values
  Buf slist, sfound, spres, sscr, smem, sval;  // split decode of large members (inflate_split.hip)
  Buf glist, gfound, gbig, gbigs, gspb, gspl, gflist, gent, gblk, glanes, gtab, gmem, gpbase, gplist, gsbase, gscr, gcnt;
  // host staging for the host-buffer entry points
  Buf d_in, d_out, d_res, d_pack, d_offs;
  HostBuf h_in, h_out, h_res, h_offs;
  hipStream_t h2d = nullptr, d2h = nullptr;  // the host entries' copies, beside the kernels (host_batch)
  std::vector<hipEvent_t> hev;               // their events, reused
  std::vector<uint8_t> hmeta;
  size_t last_n = 0;
  // timing
  struct Mark {
    std::string name;
    hipEvent_t ev;
    hipStream_t st;
  };
  std::vector<Mark> marks;  // a phase = the time between consecutive marks on the same stream
  // folded (pending) results since the last query: marks are folded in when
  // more than kMaxMarks are pending, so an unqueried timing run stays bounded
  std::vector<std::pair<std::string, double>> phase_acc;
  double total_acc = 0;
  bool acc_any = false;
  std::vector<std::pair<std::string, double>> phase_ms;  // the last query's results
  double total_ms = -1;
  // inflate lane count of the last batch: copied to pinned memory on the batch's stream, then an event
  uint32_t* lane_count_host = nullptr;
  hipEvent_t lane_ev = nullptr;
};
static constexpr size_t kMaxMarks = 1024;

// A public call starts, once per call: clears the counters that belong to its kind (include/zs_gpu.h) --
// checksum parts: any; host chunks: deflate and inflate; flush index: deflate; lane and seg counts: inflate.
enum CallKind { CALL_DEFLATE, CALL_INFLATE, CALL_CHECKSUM };
static void call_begin(zs_ctx* c, CallKind kind) {
  zs_ctx::Call& k = c->call;
  k.ck_parts = 0;
  if (kind != CALL_CHECKSUM) k.host_chunks = 0;
  if (kind == CALL_DEFLATE) {
    k.fidx.clear();
    k.fscan_at = k.fscan_used = 0;
  }
  if (kind == CALL_INFLATE) {
    k.seg_ran = k.lanes_zeroed = k.sync = k.members = false;
    k.bgzf_trusted = 0;
  }
}
static void fold_marks(zs_ctx* c);

// Phase boundary: records a timing event and, with check_phases, waits for the
// phase and reports a launch or execution error under the phase's name.
static int mark(zs_ctx* c, hipStream_t st, const char* name) {
  if (c->check_phases) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      const std::string msg = std::string(name) + ": " + hipGetErrorString(e);
      return fail(ZS_MEM_ERROR, "%s", msg.c_str());
    }
  }
  if (!c->timing) return ZS_OK;
  if (c->marks.size() >= kMaxMarks) fold_marks(c);
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return ZS_OK;
  (void)hipEventRecord(e, st);
  c->marks.push_back({name, e, st});
  return ZS_OK;
}
#define MARK(name)                              \
  do {                                          \
    const int r_ = mark(c, st, name);           \
    if (r_ != ZS_OK) return r_;                 \
  } while (0)

// Folds the pending marks into the accumulated phase times: waits for the
// last one, keeps it as the anchor of the next marks (so the time between two
// folds is not lost) and destroys the others.
static void fold_marks(zs_ctx* c) {
  if (c->marks.size() < 2) return;
  (void)hipEventSynchronize(c->marks.back().ev);
  for (size_t i = 1; i < c->marks.size(); i++) {
    size_t j = i;  // the previous mark on the same stream
    while (j-- > 0 && c->marks[j].st != c->marks[i].st) {}
    if (j == (size_t)-1) continue;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->marks[j].ev, c->marks[i].ev);
    c->phase_acc.emplace_back(c->marks[i].name, ms);
  }
  float tot = 0;
  (void)hipEventElapsedTime(&tot, c->marks.front().ev, c->marks.back().ev);
  c->total_acc += tot;
  c->acc_any = true;
  for (size_t i = 0; i + 1 < c->marks.size(); i++) (void)hipEventDestroy(c->marks[i].ev);
  c->marks.erase(c->marks.begin(), c->marks.end() - 1);
}

// Turns the marks of every batch since the last query into phase times (waits
// for the last one).  Batch calls never wait for their marks, so a timed
// sequence of batches runs back to back.
static void collect_marks(zs_ctx* c) {
  fold_marks(c);
  for (auto& m : c->marks) (void)hipEventDestroy(m.ev);
  c->marks.clear();
  if (!c->acc_any) return;  // nothing new: keep the last results
  c->phase_ms.swap(c->phase_acc);
  c->phase_acc.clear();
  c->total_ms = c->total_acc;
  c->total_acc = 0;
  c->acc_any = false;
}

// zs_set_option's table: a flag takes any value (non-zero: on); the others are
// refused with `msg` unless ok(c, value).
struct Option {
  const char* name;
  void (*set)(zs_ctx*, int);
  bool (*ok)(const zs_ctx*, int);
  const char* msg;
};
#define OPT_FLAG(nm, field) {nm, [](zs_ctx* c, int v) { c->field = v != 0; }, nullptr, nullptr}
#define OPT_INT(nm, field, cond, msg) \
  {nm, [](zs_ctx* c, int v) { c->field = (decltype(c->field))v; }, [](const zs_ctx*, int v) { return cond; }, msg}
static const Option kOptions[] = {
    OPT_FLAG("timing", timing),
    OPT_FLAG("inflate_fast", o.inflate_fast),
    OPT_FLAG("inflate_ref_wrap", o.inflate_ref_wrap),
    OPT_FLAG("check_phases", check_phases),
    OPT_FLAG("match_sweep", o.match_sweep),
    OPT_FLAG("rle_ref", o.rle_ref),
    OPT_FLAG("fast_group", fast_group),
    {"lane_order", [](zs_ctx* c, int v) { c->lane_order = v != 0; },
     [](const zs_ctx* c, int v) { return !v || c->lane_order_ok; },
     "lane_order: this device does not apply LDS atomics in lane order"},
    OPT_FLAG("inflate_split", o.inflate_split),
    OPT_FLAG("inflate_seg", o.inflate_seg),
    OPT_FLAG("seg_wide", o.seg_wide),
    OPT_INT("seg_split", o.seg_split, v >= 0 && v <= 2, "seg_split must be 0, 1 or 2 (auto)"),
    OPT_INT("seg_big_bits", o.seg_big_bits, v >= 65536, "seg_big_bits must be >= 65536"),
    {"seg_scratch_mb", [](zs_ctx* c, int v) { c->o.seg_scratch_max = (uint64_t)v << 20; },
     [](const zs_ctx*, int v) { return v >= 0; }, "seg_scratch_mb must be >= 0"},
    OPT_INT("seg_bits", o.seg_bits, v == 0 || (v >= (int)ZS_SEG_W && v <= (int)ZS_SEG_SMAX),
            "seg_bits must be 0 (auto) or 1024 .. 8192"),
    OPT_INT("seg_small_batch", o.seg_small_batch, v >= 0, "seg_small_batch must be >= 0"),
    OPT_INT("seg_small_min", o.seg_small_min, v >= 0, "seg_small_min must be >= 0"),
    OPT_INT("parse_waves", o.parse_waves, v >= 0 && v <= 4 && v != 3, "parse_waves must be 0, 1, 2 or 4"),
    OPT_INT("lane_block", o.lane_block, v == 0 || (v >= 1 && v <= 64 && !(v & (v - 1))),
            "lane_block must be 0 or a power of two <= 64"),
    OPT_INT("lane_large_min", o.lane_large_min, v >= 0, "lane_large_min must be >= 0"),
    OPT_INT("inflate_wave_min", o.inflate_wave_min, v >= 0, "inflate_wave_min must be >= 0"),
    OPT_INT("checksum_split", o.checksum_split, zs_checksum_split_ok(v), "checksum_split must be >= 0"),
    OPT_INT("checksum_part", o.checksum_part, zs_checksum_part_ok(v),
            "checksum_part must be a power of two, 1024 .. 1048576"),
    OPT_INT("host_chunk_min", o.host_chunk_min, zs_host_chunk_min_ok(v), "host_chunk_min must be >= 0"),
    OPT_INT("host_pack_min", o.host_pack_min, zs_host_pack_min_ok(v), "host_pack_min must be >= 0"),
    OPT_INT("sync_pass", o.sync_pass, zs_sync_pass_ok(v), "sync_pass must be 1 .. 64"),
};

extern "C" {

const char* zs_last_error(void) { return g_err.c_str(); }
const char* zs_version(void) { return "zs_gpu 0.1 (gfx950)"; }

int zs_ctx_create(int device, zs_ctx** out) {
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0)
    return fail(ZS_STREAM_ERROR, "no HIP device %s", std::to_string(device).c_str());
  HIPCHK(hipSetDevice(device));
  zs_ctx* c = new zs_ctx();
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return fail(ZS_MEM_ERROR, "%s", hipGetErrorString(e));
  }
  int prio_lo = 0, prio_hi = 0;  // (numerically lower = higher priority)
  if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_lo = prio_hi = 0;
  if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithPriority(&c->side2, hipStreamNonBlocking, prio_hi) != hipSuccess ||
      hipEventCreateWithFlags(&c->join2, hipEventDisableTiming) != hipSuccess ||
      hipStreamCreateWithFlags(&c->h2d, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->d2h, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->join, hipEventDisableTiming) != hipSuccess) {
    zs_ctx_destroy(c);
    return fail(ZS_MEM_ERROR, "%s", "cannot create the side stream");
  }
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
      c->o.ncu = (uint32_t)ncu;
  }
  // the chain builders use lane-ordered LDS atomics where the device applies them so:
  // check before any use; a device that violates it gets the ballot-ranked form
  uint64_t bad = 0;
  const int st = zs_selftest(c, &bad);
  if (st != ZS_OK) {
    const std::string why = zs_last_error();
    zs_ctx_destroy(c);
    return fail(ZS_STREAM_ERROR, "self-test failed: %s", why.c_str());
  }
  c->lane_order = c->lane_order_ok = bad == 0;
  *out = c;
  return ZS_OK;
}

int zs_selftest(zs_ctx* c, uint64_t* violations) {
  if (!c || !violations) return fail(ZS_STREAM_ERROR, "invalid arguments");
  *violations = 0;
  HIPCHK(hipSetDevice(c->device));
  uint32_t* d_bad = nullptr;
  HIPCHK(hipMalloc(&d_bad, sizeof(uint32_t)));
  hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(uint32_t), c->stream);
  if (e == hipSuccess) {
    zs_k_selftest<<<256, 64, 0, c->stream>>>(d_bad, 32);
    e = hipGetLastError();
  }
  uint32_t h = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d_bad, sizeof h, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_bad);
  if (e != hipSuccess) return fail(ZS_MEM_ERROR, "%s", hipGetErrorString(e));
  *violations = h;
  return ZS_OK;
}

void zs_ctx_destroy(zs_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : c->hev) (void)hipEventDestroy(e);
  for (hipStream_t q : {c->h2d, c->d2h})
    if (q) {
      (void)hipStreamSynchronize(q);
      (void)hipStreamDestroy(q);
    }
  for (auto& m : c->marks) (void)hipEventDestroy(m.ev);
  if (c->lane_ev) (void)hipEventSynchronize(c->lane_ev);
  if (c->lane_count_host) (void)hipHostFree(c->lane_count_host);
  if (c->lane_ev) (void)hipEventDestroy(c->lane_ev);
  if (c->side) (void)hipStreamSynchronize(c->side);
  if (c->fork) (void)hipEventDestroy(c->fork);
  if (c->join) (void)hipEventDestroy(c->join);
  if (c->side2) (void)hipStreamSynchronize(c->side2);
  if (c->join2) (void)hipEventDestroy(c->join2);
  if (c->side2) (void)hipStreamDestroy(c->side2);
  if (c->side) (void)hipStreamDestroy(c->side);
  (void)hipStreamDestroy(c->stream);
  delete c;  // (frees the workspace and staging buffers)
}

void zs_set_timing(zs_ctx* c, int on) { c->timing = on != 0; }

int zs_set_option(zs_ctx* c, const char* name, int value) {
  if (!c || !name) return fail(ZS_STREAM_ERROR, "invalid arguments");
  for (const Option& o : kOptions) {
    if (strcmp(name, o.name)) continue;
    if (o.msg && !o.ok(c, value)) return fail(ZS_STREAM_ERROR, "%s", o.msg);
    o.set(c, value);
    return ZS_OK;
  }
  return fail(ZS_STREAM_ERROR, "unknown option %s", name);
}
double zs_last_batch_ms(zs_ctx* c) {
  collect_marks(c);
  return c->total_ms;
}
uint32_t zs_last_inflate_lane_count(zs_ctx* c) {
  if (!c || !c->lane_count_host || hipEventSynchronize(c->lane_ev) != hipSuccess) return 0;
  return *(volatile uint32_t*)c->lane_count_host;
}
uint32_t zs_last_inflate_seg_count(zs_ctx* c) {
  uint32_t v = 0;
  if (!c || !c->call.seg_ran || !c->gcnt.p || hipStreamSynchronize(c->side) != hipSuccess ||
      hipMemcpy(&v, c->gcnt.as<uint32_t>() + 1, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  return v;
}
uint32_t zs_last_checksum_parts(zs_ctx* c) { return c ? c->call.ck_parts : 0u; }
uint32_t zs_last_host_chunks(zs_ctx* c) { return c ? c->call.host_chunks : 0u; }
double zs_last_phase_ms(zs_ctx* c, const char* phase) {
  collect_marks(c);
  double t = -1;
  for (auto& p : c->phase_ms)
    if (p.first == phase) t = (t < 0 ? 0 : t) + p.second;
  return t;
}

// zlib's crc32_combine: crc32(A) x^(8 |B|) + crc32(B) modulo the reflected polynomial, the power
// from x^(2^j) by squaring (x^(2^32) = x: the exponent's bits above 31 wrap round)
static uint32_t multmodp(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
  }
  return p;
}
uint32_t zs_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
  if (!len2) return crc1;
  uint32_t x2 = 1u << 30, p = 1u << 31;  // x^(2^j), j = 0; x^0
  for (int j = 0; j < 3; j++) x2 = multmodp(x2, x2);  // bytes: x^8
  for (uint64_t e = len2; e; e >>= 1, x2 = multmodp(x2, x2))
    if (e & 1) p = multmodp(x2, p);
  return multmodp(p, crc1) ^ crc2;
}
// zlib's adler32_combine: with A1, B1 and A2, B2 the halves, A = A1 + A2 - 1 and
// B = B1 + B2 + |B| (A1 - 1) (mod 65521)
uint32_t zs_adler32_combine(uint32_t adler1, uint32_t adler2, uint64_t len2) {
  if (!len2) return adler1;
  const uint64_t base = 65521, rem = len2 % base;
  const uint64_t a1 = adler1 & 0xffffu, b1 = adler1 >> 16, a2 = adler2 & 0xffffu, b2 = adler2 >> 16;
  const uint64_t a = (a1 + a2 + base - 1) % base;
  const uint64_t b = (rem * a1 + b1 + b2 + base - rem) % base;
  return (uint32_t)(b << 16 | a);
}

uint64_t zs_deflate_bound(uint64_t n, int wbits) {  // deflate.ts:615-674, memLevel 8 / windowBits 15
  const uint64_t wraplen = wbits < 0 ? 0 : (wbits > 15 ? 18 : 6);
  const uint64_t b = n + (n >> 12) + (n >> 14) + (n >> 25) + 13 - 6 + wraplen;
  return b;  // (output capacities must still be multiples of 4: round up when allocating)
}

// deflate.ts:619-673 for deflateInit2_'s windowBits and memLevel
uint64_t zs_deflate_bound_params(uint64_t n, int wbits, int mem_level, int level) {
  int wrap;
  const int wb = zs_wbits_split(wbits, &wrap);
  if (!wb || mem_level < 1 || mem_level > 9) return 0;
  const zs_deflate_params q = zs_make_params(wb, mem_level);
  const uint64_t wraplen = wrap == 0 ? 0 : wrap == 1 ? 6 : 18;
  if (q.w_bits != 15 || q.hash_bits != 8 + 7) {  // deflate.ts:669-671
    const uint64_t fixedlen = n + (n >> 3) + (n >> 8) + (n >> 9) + 4;
    const uint64_t storelen = n + (n >> 5) + (n >> 7) + (n >> 11) + 7;
    return (q.w_bits <= q.hash_bits && level ? fixedlen : storelen) + wraplen;
  }
  return zs_deflate_bound(n, wrap == 0 ? -15 : wrap == 1 ? 15 : 31);
}

uint64_t zs_deflate_bound_dict(uint64_t n, int wbits, uint64_t dict_len) {  // deflate.ts:633: DICTID (zlib, strstart != 0)
  return zs_deflate_bound(n, wbits) + (wbits == 15 && dict_len ? 4u : 0u);
}

}  // extern "C"

// A batch's arrays: the data pointers (device memory) and the per-stream offsets,
// lengths and capacities -- host arrays as an entry point receives them, device
// arrays (in c->meta) as upload_batch returns them.
struct Batch {
  uint32_t n;
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* in_len;
  uint8_t* out;
  const uint64_t* out_off;
  const uint32_t* out_cap;
};

// The preset dictionaries of a batch: the bytes (device memory; the caller's host memory on the
// way into deflate_host), host arrays of the members' offsets and lengths (length 0: none)
struct DictIn {
  const uint8_t* d_dict;
  const uint64_t* off;
  const uint32_t* len;
};

// Fills the host copy of the metadata block (`bytes` of it) from h's host arrays
// (the output arrays may be null) and with fill(block) for whatever else it holds,
// grows c->meta, uploads the block on st and returns the batch with device arrays.
template <class Fill>
static int upload_batch(zs_ctx* c, hipStream_t st, const zs_meta_layout& ml, size_t bytes, const Batch& h, Batch* d,
                        Fill fill) {
  c->hmeta.resize(bytes);
  c->last_n = h.n;
  uint8_t* hm = c->hmeta.data();
  memcpy(hm + ml.in_off, h.in_off, 8ull * h.n);
  memcpy(hm + ml.in_len, h.in_len, 4ull * h.n);
  if (h.out_off) memcpy(hm + ml.out_off, h.out_off, 8ull * h.n);
  if (h.out_cap) memcpy(hm + ml.out_cap, h.out_cap, 4ull * h.n);
  fill(hm);
  HIPCHK(c->meta.ensure(bytes));
  HIPCHK(hipMemcpyAsync(c->meta.p, hm, bytes, hipMemcpyHostToDevice, st));
  const uint8_t* dm = c->meta.as<uint8_t>();
  *d = {h.n, h.in, (const uint64_t*)(dm + ml.in_off), (const uint32_t*)(dm + ml.in_len), h.out,
        (const uint64_t*)(dm + ml.out_off), (const uint32_t*)(dm + ml.out_cap)};
  return ZS_OK;
}

// The data checksum of a batch (the deflate wrappers' check values, the checksum entries, the
// inflate trailer check), in three steps around upload_batch: ck_prepare plans it from the
// lengths' bounds, adds its parts to the call's record and returns the plan and the bytes its part
// map takes behind the metadata block -- no plan and no bytes for a batch that wants none; ck_fill
// writes the map there; ck_launch runs it -- one wave per stream as ever, or the parts and the fold.
static int ck_prepare(zs_ctx* c, bool want, uint32_t n, const uint32_t* len_bound, const zs_checksum_plan** plan,
                      size_t* map_bytes) {
  *plan = nullptr;
  *map_bytes = 0;
  if (!want) return ZS_OK;
  zs_plan_checksum(c->o, n, len_bound, c->cp);
  c->call.ck_parts += c->cp.P;
  *plan = &c->cp;
  *map_bytes = c->cp.map_bytes();
  HIPCHK(c->ckvals.ensure(c->cp.ws_bytes));
  return ZS_OK;
}
static void ck_fill(const zs_checksum_plan* cp, uint8_t* map) {
  if (!cp || !cp->split) return;
  memcpy(map, cp->pfirst.data(), 4ull * cp->pfirst.size());
  memcpy(map + cp->map_pstream(), cp->pstream.data(), 4ull * cp->P);
}
// ck: the batch's plan as ck_prepare returned it; map: the part map's place in c->meta (a split plan);
// in_off, in_len, seeds: device arrays
static void ck_launch(zs_ctx* c, hipStream_t st, const zs_checksum_plan& cp, size_t map, uint32_t n, const uint8_t* in,
                      const uint64_t* in_off, const uint32_t* in_len, uint32_t* check, int kind,
                      const uint32_t* seeds = nullptr) {
  if (!cp.split) {
    zs_k_checksum<<<n, 64, 0, st>>>(in, in_off, in_len, check, kind, seeds);
    return;
  }
  const uint32_t* pfirst = (const uint32_t*)(c->meta.as<uint8_t>() + map);
  const uint32_t* pstream = (const uint32_t*)(c->meta.as<uint8_t>() + map + cp.map_pstream());
  uint32_t* vals = c->ckvals.as<uint32_t>();
  zs_k_checksum_parts<<<cp.P, 64, 0, st>>>(in, in_off, in_len, pfirst, pstream, cp.part_lg, vals, kind);
  zs_k_checksum_fold<<<n, 64, 0, st>>>(in_len, pfirst, cp.part_lg, vals, check, kind, seeds);
}

__global__ void zs_k_finish(const zs_stream* streams, int32_t* status, uint32_t* out_len, int n) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  status[s] = streams[s].status;
  out_len[s] = streams[s].status == ZS_Z_STREAM_END ? streams[s].out_len : 0u;
}

__global__ void zs_k_copy_check(const uint32_t* check, zs_stream* streams, int n) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) streams[s].check = check[s];
}

// zs_deflate_validate's findings, as the entries report them
static int deflate_fail(zs_deflate_err e) {
  static const char* const kMsg[ZS_DE_COUNT] = {
      "",
      "unsupported windowBits (use -15, 15 or 31)",
      "invalid level",
      "invalid strategy",
      "invalid window bits",
      "invalid memLevel",
      "null dictionary arrays",
      "null dictionary buffer",
      "dictionaries are for deflate-raw (-15) and zlib (15) only",
      "level 0 with a preset dictionary is not built",
      "stream too long for a preset dictionary",
      "level 0 with non-default windowBits / memLevel is not built",
      "stream too long for Z_RLE",
      "output offsets/capacities must be multiples of 4",
      "a preset dictionary with a strategy or windowBits / memLevel is not built",
      "flush mode not built",
      "invalid flush",
      "null flush arrays",
      "invalid flush positions",
      "level 0 with a flush point is not built",
      "too many flush points (streams + flush points above 65,535 in one call)",
      "invalid BGZF block size",
      "null arrays",
      "too many BGZF blocks (streams + blocks above 65,535 in one call)",
  };
  return fail(ZS_STREAM_ERROR, "%s", kMsg[e]);
}

// ---- the kernel instances of a deflate batch, by the plan's coordinates (zs_plan.h)
typedef decltype(&zs_k_parse) parse_fn;
typedef decltype(&zs_k_parse_dict) parse_dict_fn;
typedef decltype(&zs_k_parse_par) parse_par_fn;
typedef decltype(&zs_k_fast<2, true, false>) fast_fn;
typedef decltype(&zs_k_fast_par<2, true, false>) fast_par_fn;
static int pw_index(int pw) { return pw == 4 ? 2 : pw == 2 ? 1 : 0; }
static int nice_index(int bucket) { return bucket == 8 ? 2 : bucket == 4 ? 1 : 0; }
// the lazy parse (deflate_parse.hip): one, two or four waves per stream
static parse_fn parse_kernel(zs_variant v, int pw) {
  static const parse_fn k[2][3] = {{zs_k_parse, zs_k_parse_2w, zs_k_parse_4w},
                                   {zs_k_parse_filt, zs_k_parse_2w_filt, zs_k_parse_4w_filt}};
  return k[v == ZS_VAR_FILT][pw_index(pw)];
}
static parse_dict_fn parse_dict_kernel(int pw) {
  static const parse_dict_fn k[3] = {zs_k_parse_dict, zs_k_parse_2w_dict, zs_k_parse_4w_dict};
  return k[pw_index(pw)];
}
static parse_par_fn parse_par_kernel(int pw) {
  static const parse_par_fn k[3] = {zs_k_parse_par, zs_k_parse_2w_par, zs_k_parse_4w_par};
  return k[pw_index(pw)];
}
// levels 1..3: the group-speculative replay or the step-by-step one; [nice bucket][lane_order]
#define ZS_FAST_INSTANCES(K, D) {{K<2, false, D>, K<2, true, D>}, {K<4, false, D>, K<4, true, D>}, {K<8, false, D>, K<8, true, D>}}
static fast_fn fast_kernel(zs_sym_route route, bool dict, int nice_bucket, bool lane_order) {
  static const fast_fn group[2][3][2] = {ZS_FAST_INSTANCES(zs_k_fast, false), ZS_FAST_INSTANCES(zs_k_fast, true)};
  static const fast_fn serial[2] = {zs_k_fast_serial<false>, zs_k_fast_serial<true>};
  return route == ZS_SYM_FAST_GROUP ? group[dict][nice_index(nice_bucket)][lane_order] : serial[dict];
}
static fast_par_fn fast_par_kernel(int nice_bucket, bool lane_order) {
  static const fast_par_fn k[3][2] = ZS_FAST_INSTANCES(zs_k_fast_par, false);
  return k[nice_index(nice_bucket)][lane_order];
}
#undef ZS_FAST_INSTANCES

// The deflate launch sequence of a batch b (planned in p, its metadata uploaded) on
// stream st: the stored blocks (level 0); else the match finding (levels 4..9) and
// the parse, or deflate_fast (1..3), or a strategy's tally; then trees, layout, emit,
// wrapper, statuses.  (A pipeline of chunks of streams -- chunk j's parse .. emit on a
// side stream beside chunk j + 1's sweep -- measured slower twice: DESIGN 5,
// tools/variants/r05_paths.patch.)
// A batch with preset dictionaries (p.dict): b holds the JOINED streams (dictionary tail + data,
// DESIGN 4.6), `data` the caller's data (the check values are over the data alone; else data is b);
// the parse starts at the streams' parse starts, the zlib wrapper carries FDICT / DICTID.
// A batch with flush points (fl): b holds the SEGMENTS (b.out_off the segment's stream's),
// `data` the streams, whose check values, layout scan, wrapper and results are per stream.
// A primed batch (p.req.primed) is both: b holds the segments' J -- the prime, then the piece, read
// where they lie in the caller's input -- the DICT instances parse them from d_start on, and the flushed layout,
// the plain wrapper and the streams' results follow.  The blocks' in_start / in_end are J's coordinates, as
// b.in_off is, and the layout kernels read their difference alone: they take no d_start.
struct FlushDev {
  const uint32_t* sfirst;   // device: each stream's first segment
  const uint32_t* sstream;  // ... each segment's stream
  uint32_t bgzf = 0;        // a BGZF batch's block size: the segments are finished members
};
// The layout of a BGZF batch of M segments and n streams (deflate_bgzf.hip); M may be 0: end-of-file blocks alone
static void bgzf_layout(zs_ctx* c, hipStream_t st, const FlushDev& fl, const uint32_t* d_blk, zs_block* d_bk,
                        zs_stream* d_st, zs_stream* d_res, const Batch& data, uint32_t M) {
  const uint32_t tiles = M / ZS_FLUSH_TILE + 1;
  uint64_t* segx = c->fscan.as<uint64_t>() + c->call.fscan_at;
  uint64_t* tile = segx + M + 1;
  zs_k_bgzf_local<<<tiles, ZS_FLUSH_TILE, 0, st>>>(d_blk, d_bk, d_st, fl.sstream, d_res, segx, tile, M);
  zs_k_flush_tiles<<<1, ZS_FLUSH_TILE, 0, st>>>(tile, tiles);
  zs_k_bgzf_place<<<std::max(M, data.n) / ZS_FLUSH_TILE + 1, ZS_FLUSH_TILE, 0, st>>>(
      d_blk, d_bk, d_st, fl.sfirst, fl.sstream, d_res, segx, tile, data.out_cap, data.out, data.out_off, M, data.n);
}
static int deflate_launch(zs_ctx* c, hipStream_t st, const zs_deflate_plan& p, const Batch& b, const Batch& data,
                          int32_t* d_status, uint32_t* d_out_len, const zs_checksum_plan* ck, size_t ck_map,
                          const FlushDev* fl = nullptr) {
  const zs_level_cfg& cfg = zs_level_cfgs[p.cfg];
  const zs_meta_layout& ml = p.ml;
  const bool bgzf = fl && fl->bgzf;
  // (a BGZF batch's segments are raw streams to the kernels; the gzip frames are zs_k_bgzf_frame's)
  const int wrap = bgzf ? 0 : p.req.wrap, level = p.req.level;
  const bool par = p.variant == ZS_VAR_PAR;  // non-default windowBits / memLevel: the *_par instances
  const zs_kpar kp = p.req.q.kpar();
  const uint32_t n = p.n;
  const uint8_t* dm = c->meta.as<uint8_t>();
  const uint64_t* d_pos = (const uint64_t*)(dm + ml.pos_base);
  const uint32_t* d_blk = (const uint32_t*)(dm + ml.blk_base);
  const zs_sweep_seg* d_segs = (const zs_sweep_seg*)(dm + ml.segs);
  const uint32_t* d_start = p.dict ? (const uint32_t*)(dm + ml.start) : nullptr;
  zs_stream* d_st = c->streams.as<zs_stream>();
  // the records the check values, the wrapper and the results go by: the streams', n_res of them
  zs_stream* d_res = fl ? c->fstreams.as<zs_stream>() : d_st;
  const uint32_t n_res = data.n;
  zs_block* d_bk = c->blocks.as<zs_block>();
  uint32_t* syms = c->syms.as<uint32_t>();
  uint32_t* check = c->check.as<uint32_t>();
  const int nthreads_s = 256, nblocks_s = (int)p.g_streams;
  const int nblocks_r = (int)((n_res + 255) / 256);
  MARK("start");
  if (fl && !p.stored) HIPCHK(hipMemsetAsync(d_res, 0, sizeof(zs_stream) * (size_t)n_res, st));
  if (bgzf) {
    // the streams' crc32 (check[i]: what a reader that concatenates the members computes), and behind them
    // the members' own -- one wave each: a piece is far below any parts threshold
    uint32_t* seg_check = check + n_res;
    ck_launch(c, st, *ck, ck_map, n_res, data.in, data.in_off, data.in_len, check, 2);
    if (n) zs_k_checksum<<<n, 64, 0, st>>>(b.in, b.in_off, b.in_len, seg_check, 2);
    MARK("checksum");
    if (p.stored) {
      const uint32_t member = fl->bgzf + ZS_BGZF_HEADER + 5 + ZS_BGZF_TRAILER;
      zs_k_bgzf_stored<<<dim3(member / 4096 + 1, n + n_res), 256, 0, st>>>(
          b.in, b.in_off, b.in_len, seg_check, fl->sfirst, fl->sstream, data.in_len, data.out, data.out_off,
          data.out_cap, fl->bgzf, n, d_status, d_out_len);
      MARK("stored");
      return ZS_OK;
    }
    zs_k_copy_check<<<nblocks_r, nthreads_s, 0, st>>>(check, d_res, (int)n_res);
    if (n == 0) {  // every stream is empty: end-of-file blocks alone
      bgzf_layout(c, st, *fl, d_blk, d_bk, d_st, d_res, data, 0);
      MARK("layout");
      zs_k_bgzf_frame<<<n_res / 256 + 1, 256, 0, st>>>(d_st, fl->sstream, d_res, b.in_len, seg_check, data.out,
                                                       data.out_off, 0, n_res);
      MARK("bgzf_frame");
      zs_k_finish<<<nblocks_r, nthreads_s, 0, st>>>(d_res, d_status, d_out_len, (int)n_res);
      MARK("finish");
      return ZS_OK;
    }
  }
  if (p.stored) {
    if (wrap) {
      ck_launch(c, st, *ck, ck_map, n, b.in, b.in_off, b.in_len, check, wrap == 1 ? 1 : 2);
      MARK("checksum");
    }
    zs_k_stored<<<dim3(p.g_stored_x, n), 256, 0, st>>>(b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, check, wrap,
                                                       d_status, d_out_len);
    MARK("stored");
    return ZS_OK;
  }
  if (wrap) {
    ck_launch(c, st, *ck, ck_map, n_res, data.in, data.in_off, data.in_len, check, wrap == 1 ? 1 : 2);
    zs_k_copy_check<<<nblocks_r, nthreads_s, 0, st>>>(check, d_res, (int)n_res);
    MARK("checksum");
  }
  if (p.match == ZS_MATCH_SWEEP) {
    const uint32_t nw = (uint32_t)p.segs.size();
    // a window: counting sort by hash + lock-step sweep (deflate_sweep.hip)
    (p.lane_order ? zs_k_bucket<true> : zs_k_bucket<false>)<<<nw, ZS_BK_THREADS, 0, st>>>(
        b.in, b.in_off, b.in_len, d_pos, d_segs, c->prevd.as<uint16_t>(), c->mres.as<uint2>());
    MARK("bucket");
    // (a chain budget that is not all groups of eight falls back to the general walk)
    (p.sweep_u8 ? zs_k_sweep<true> : zs_k_sweep<false>)<<<nw, 1024, 0, st>>>(
        b.in, b.in_off, b.in_len, d_pos, d_segs, c->prevd.as<uint16_t>(), c->mres.as<uint2>(), cfg.chain, cfg.nice);
    MARK("sweep");
  } else if (p.match == ZS_MATCH_CHAIN) {
    // the chain-walk kernels: a cross-check of the sweep (option match_sweep = 0), or with the runtime
    // window and hash (they follow prev[] links whatever the hash)
    const dim3 g(p.g_match_x, n);
    if (par) (p.lane_order ? zs_k_prev_par<true> : zs_k_prev_par<false>)<<<n, 64, 0, st>>>(b.in, b.in_off, b.in_len, d_pos,
                                                                                             c->prevd.as<uint16_t>(), 0u, kp);
    else (p.lane_order ? zs_k_prev<true> : zs_k_prev<false>)<<<n, 64, 0, st>>>(b.in, b.in_off, b.in_len, d_pos,
                                                                                c->prevd.as<uint16_t>(), 0u);
    MARK("prev");
    if (p.max_len && par) zs_k_match_par<<<g, 1024, 0, st>>>(b.in, b.in_off, b.in_len, d_pos, c->prevd.as<uint16_t>(),
                                                              c->mres.as<uint2>(), cfg.chain, cfg.nice, 0u, kp);
    else if (p.max_len) zs_k_match<<<g, 1024, 0, st>>>(b.in, b.in_off, b.in_len, d_pos, c->prevd.as<uint16_t>(),
                                                        c->mres.as<uint2>(), cfg.chain, cfg.nice, 0u);
    MARK("match");
  }
  switch (p.sym) {
    case ZS_SYM_HUFF:
      zs_k_huff_tally<<<(uint32_t)p.chunks.size(), 256, 0, st>>>(b.in, b.in_off, b.in_len, d_pos, d_blk,
                                                                 (const zs_huff_chunk*)(dm + ml.chunks), syms, d_bk, d_st);
      MARK("huff_tally");
      break;
    case ZS_SYM_RLE:
      zs_k_rle_tally<<<n, 256, 0, st>>>(b.in, b.in_off, b.in_len, d_pos, d_blk, syms, d_bk, d_st);
      MARK("rle_tally");
      break;
    case ZS_SYM_PARSE:  // the lazy parse (deflate_parse.hip), p.pw waves per stream
      if (par)
        parse_par_kernel(p.pw)<<<n, 64 * p.pw, 0, st>>>(b.in, b.in_off, b.in_len, d_pos, d_blk, c->mres.as<uint2>(), syms,
                                                        d_bk, d_st, c->pscr.as<uint32_t>(), cfg.good, cfg.lazy, kp);
      else if (p.dict)
        parse_dict_kernel(p.pw)<<<n, 64 * p.pw, 0, st>>>(b.in, b.in_off, b.in_len, d_pos, d_blk, c->mres.as<uint2>(), syms,
                                                         d_bk, d_st, c->pscr.as<uint32_t>(), cfg.good, cfg.lazy, d_start);
      else
        parse_kernel(p.variant, p.pw)<<<n, 64 * p.pw, 0, st>>>(b.in, b.in_off, b.in_len, d_pos, d_blk, c->mres.as<uint2>(),
                                                               syms, d_bk, d_st, c->pscr.as<uint32_t>(), cfg.good, cfg.lazy);
      MARK("parse");
      break;
    default:  // levels 1..3 (deflate_fast.hip): the instance and its LDS by the tables' sizes (zs_plan_fast_params)
      if (!par) {
        const fast_fn fast = fast_kernel(p.sym, p.dict, p.nice_bucket, p.lane_order);
        HIPCHK(hipFuncSetAttribute((const void*)fast, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.fast_lds));
        fast<<<n, 64, p.fast_lds, st>>>(b.in, b.in_off, b.in_len, d_pos, d_blk, syms, d_bk, d_st, cfg.chain, cfg.lazy,
                                        cfg.nice, d_start);
      } else if (p.sym == ZS_SYM_FAST_GROUP) {
        const fast_par_fn fast = fast_par_kernel(p.nice_bucket, p.lane_order);
        HIPCHK(hipFuncSetAttribute((const void*)fast, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.fast_lds));
        fast<<<n, 64, p.fast_lds, st>>>(b.in, b.in_off, b.in_len, d_pos, d_blk, syms, d_bk, d_st, cfg.chain, cfg.lazy,
                                        cfg.nice, nullptr, kp);
      } else {
        uint16_t* gh = p.sym == ZS_SYM_FAST_SERIAL_GHEAD ? c->ghead.as<uint16_t>() : nullptr;
        const auto fast = gh ? zs_k_fast_serial_par<false, true> : zs_k_fast_serial_par<false, false>;
        HIPCHK(hipFuncSetAttribute((const void*)fast, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.fast_lds));
        fast<<<n, 64, p.fast_lds, st>>>(b.in, b.in_off, b.in_len, d_pos, d_blk, syms, d_bk, d_st, cfg.chain, cfg.lazy,
                                        cfg.nice, nullptr, kp, gh);
      }
      MARK("fast");
  }
  (par ? zs_k_trees_par : zs_k_trees)<<<dim3(p.max_blk, n), 64, 0, st>>>(
      b.in, b.in_off, d_pos, d_blk, syms, d_bk, d_st, c->codes.as<uint32_t>(), c->hdr.as<uint32_t>(), (int)n,
      p.fixed ? 1 : 0);
  MARK("trees");
  if (p.dict && !fl) zs_k_layout_dict<<<nblocks_s, nthreads_s, 0, st>>>(d_blk, d_bk, d_st, b.out_cap, b.out, b.out_off, wrap, (int)n,
                                                                 d_start);
  else if (bgzf) bgzf_layout(c, st, *fl, d_blk, d_bk, d_st, d_res, data, n);
  else if (fl) {
    // per segment, joined by a scan of the segments' bytes (deflate_flush.hip)
    const zs_flush_layout fo(ml.bytes, n_res, n);
    uint64_t* segx = c->fscan.as<uint64_t>() + c->call.fscan_at;
    uint64_t* tile = segx + n + 1;
    zs_k_flush_local<<<fo.tiles, ZS_FLUSH_TILE, 0, st>>>(d_blk, d_bk, d_st, fl->sfirst, fl->sstream, d_res, segx, tile, n);
    zs_k_flush_tiles<<<1, ZS_FLUSH_TILE, 0, st>>>(tile, fo.tiles);
    zs_k_flush_place<<<fo.tiles, ZS_FLUSH_TILE, 0, st>>>(d_blk, d_bk, d_st, fl->sfirst, fl->sstream, d_res, segx, tile,
                                                         data.out_cap, data.out, data.out_off, wrap, n);
  } else zs_k_layout<<<nblocks_s, nthreads_s, 0, st>>>(d_blk, d_bk, d_st, b.out_cap, b.out, b.out_off, wrap, (int)n);
  MARK("layout");
  zs_k_emit<<<dim3(p.max_blk, n), 256, 0, st>>>(b.in, b.in_off, d_pos, d_blk, syms, d_bk, d_st,
                                                c->codes.as<uint32_t>(), c->hdr.as<uint32_t>(), b.out, b.out_off, wrap);
  MARK("emit");
  if (bgzf) {
    zs_k_bgzf_frame<<<(n + n_res) / 256 + 1, 256, 0, st>>>(d_st, fl->sstream, d_res, b.in_len, check + n_res, data.out,
                                                           data.out_off, n, n_res);
    MARK("bgzf_frame");
  }
  if (wrap && p.dict && !fl)
    zs_k_wrap_dict<<<nblocks_s, nthreads_s, 0, st>>>(d_st, b.out, b.out_off, b.in_len, wrap, level, (int)n, d_start,
                                                     (const uint32_t*)(dm + ml.did), c->dadler.as<uint32_t>());
  else if (wrap && par)
    zs_k_wrap_par<<<nblocks_s, nthreads_s, 0, st>>>(d_st, b.out, b.out_off, b.in_len, wrap, level, (int)n,
                                                    p.wrap_strategy, p.req.q.w_bits);
  else if (wrap)
    zs_k_wrap<<<nblocks_r, nthreads_s, 0, st>>>(d_res, data.out, data.out_off, data.in_len, wrap, level, (int)n_res,
                                                p.wrap_strategy);
  zs_k_finish<<<nblocks_r, nthreads_s, 0, st>>>(d_res, d_status, d_out_len, (int)n_res);
  MARK("finish");
  return ZS_OK;
}

// Per-stream check value (the reference's strm.adler after the stream,
// deflate.ts:155-159,462,778,788): adler32 (zlib) / crc32 (gzip) of the input,
// 1 for deflate-raw (adler32(0), never updated without a wrapper); 0 for a
// stream that failed.
__global__ void zs_k_deflate_check(const int32_t* status, const uint32_t* check, int wrap, uint32_t* out, int n) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  out[s] = status[s] != ZS_Z_STREAM_END ? 0u : wrap ? check[s] : 1u;
}

// The device compress: validate (zs_deflate_validate), then plan, ensure, upload, launch, check values
// (deflate_batch).  out_cap[i] is the stream's capacity as the caller set it (Z_BUF_ERROR past it,
// exactly); the kernels store whole dwords, so the stream's region must reach out_off[i] + out_cap[i]
// rounded up to 4: `caller_regions` (the public device entries' own buffers) with capacities that are
// multiples of 4, or the host entries' staging.
// `dict`, `flush` (requests with req.dict / req.flush, else null): the streams' preset dictionaries /
// flush positions; a batch with none of them set is the plain batch.
struct FlushIn {
  const uint64_t* first;  // host, n + 1 entries: stream i's positions are pos[first[i] .. first[i + 1])
  const uint32_t* pos;    // host
};
// The arrays of a call as validation reads them
static zs_deflate_call deflate_call(const Batch& h, bool caller_regions, const DictIn* dict, const FlushIn* flush) {
  zs_deflate_call a;
  a.flush_first = flush ? flush->first : nullptr;
  a.flush_pos = flush ? flush->pos : nullptr;
  a.n = h.n;
  a.in_len = h.in_len;
  a.out_off = h.out_off;
  a.out_cap = h.out_cap;
  a.caller_regions = caller_regions;
  a.dict_arrays = dict && dict->off && dict->len;
  a.dict_buf = dict && dict->d_dict;
  a.dict_len = a.dict_arrays ? dict->len : nullptr;
  return a;
}
// The workspace of a planned batch of p.n streams (a flushed batch's segments)
static int deflate_ensure(zs_ctx* c, const zs_deflate_plan& p) {
  if (p.stored) return ZS_OK;
  HIPCHK(c->ghead.ensure(p.ghead_bytes));
  if (p.dict && !p.req.primed) {  // (a primed batch's J are slices of the input: no join, no DICTID)
    HIPCHK(c->djoin.ensure(p.J + 16));
    HIPCHK(c->dadler.ensure(4ull * p.ndict));
  }
  if (p.sym != ZS_SYM_HUFF && p.sym != ZS_SYM_RLE) {  // (the tallies search no matches)
    HIPCHK(c->prevd.ensure(p.prevd_bytes));
    HIPCHK(c->mres.ensure(p.mres_bytes));
  }
  HIPCHK(c->syms.ensure(p.syms_bytes));
  HIPCHK(c->pscr.ensure(p.pscr_bytes));
  HIPCHK(c->blocks.ensure(sizeof(zs_block) * (size_t)p.B));
  HIPCHK(c->streams.ensure(sizeof(zs_stream) * (size_t)p.n));
  HIPCHK(c->codes.ensure(p.codes_bytes));
  HIPCHK(c->hdr.ensure(p.hdr_bytes));
  return ZS_OK;
}
// ... and what follows its launch: the n streams' check values and the "end" mark
static int deflate_finish(zs_ctx* c, hipStream_t st, const zs_deflate_plan& p, uint32_t n, const int32_t* d_status,
                          uint32_t* d_check) {
  if (d_check)
    zs_k_deflate_check<<<(n + 255) / 256, 256, 0, st>>>(d_status, c->check.as<uint32_t>(), p.req.wrap, d_check, (int)n);
  if (!p.stored) MARK("end");  // (a stored batch ends at its "stored" mark)
  HIPCHK(hipGetLastError());
  return ZS_OK;  // timing marks are collected when queried (no wait here)
}
static int deflate_batch_flush(zs_ctx* c, const zs_deflate_req& req, const Batch& h, int32_t* d_status,
                               uint32_t* d_out_len, uint32_t* d_check, hipStream_t st, const FlushIn& flush);
static int deflate_batch_bgzf(zs_ctx* c, const zs_deflate_req& req, const Batch& h, int32_t* d_status,
                              uint32_t* d_out_len, uint32_t* d_check, hipStream_t st);
// A validated, non-empty device batch (a public call's, or a chunk of a host call): plan, ensure, upload, launch.
static int deflate_batch(zs_ctx* c, const zs_deflate_req& req_in, const zs_deflate_call& a, const Batch& h,
                         int32_t* d_status, uint32_t* d_out_len, uint32_t* d_check, hipStream_t st, const DictIn* dict,
                         const FlushIn* flush) {
  if (zs_deflate_any_flush(req_in, a)) return deflate_batch_flush(c, req_in, h, d_status, d_out_len, d_check, st, *flush);
  if (req_in.bgzf) return deflate_batch_bgzf(c, req_in, h, d_status, d_out_len, d_check, st);
  zs_deflate_req req = req_in;
  req.flush = 0;  // no flush point: the plain batch's plan, kernels and bytes
  req.primed = false;
  const uint32_t n = h.n;
  // the plan (host-side): routes, instances, grids, workspace bases, the sweep's windows and the
  // metadata block; the streams' dictionaries, the distinct ones found once
  zs_dict_set& ds = c->dset;
  ds.any = false;
  if (req.dict) zs_dict_distinct(n, dict->off, dict->len, ds);
  zs_deflate_plan& p = c->dp;
  zs_plan_deflate(req, c->o, c->fast_group, c->lane_order, n, h.in_len, ds.any ? dict->len : nullptr,
                  (uint32_t)ds.uoff.size(), p);
  const zs_meta_layout& ml = p.ml;
  HIPCHK(c->check.ensure(4ull * n));
  // the check values' part map behind the block (a raw batch has none)
  const zs_checksum_plan* ck;
  size_t ck_bytes;
  if (const int rc = ck_prepare(c, req.wrap != 0, n, h.in_len, &ck, &ck_bytes)) return rc;
  if (const int rc = deflate_ensure(c, p)) return rc;
  Batch b;
  int r = upload_batch(c, st, ml, ml.bytes + ck_bytes, h, &b, [&](uint8_t* hm) {
    ck_fill(ck, hm + ml.bytes);
    if (p.stored) return;
    memcpy(hm + ml.pos_base, p.pos.data(), 8ull * n);
    memcpy(hm + ml.blk_base, p.blk.data(), 4ull * n);
    if (!p.segs.empty()) memcpy(hm + ml.segs, p.segs.data(), sizeof(zs_sweep_seg) * p.segs.size());
    if (!p.chunks.empty()) memcpy(hm + ml.chunks, p.chunks.data(), sizeof(zs_huff_chunk) * p.chunks.size());
    if (!p.dict) return;
    memcpy(hm + ml.doff, dict->off, 8ull * n);
    memcpy(hm + ml.dlen, dict->len, 4ull * n);
    memcpy(hm + ml.did, ds.id.data(), 4ull * n);
    memcpy(hm + ml.start, p.start.data(), 4ull * n);
    memcpy(hm + ml.joff, p.joff.data(), 8ull * n);
    uint32_t* jl = (uint32_t*)(hm + ml.jlen);
    for (uint32_t i = 0; i < n; i++) jl[i] = p.start[i] + h.in_len[i];
    memcpy(hm + ml.uoff, ds.uoff.data(), 8ull * p.ndict);
    memcpy(hm + ml.ulen, ds.ulen.data(), 4ull * p.ndict);
  });
  if (r != ZS_OK) return r;
  if (p.dict) {
    // the joined streams take the data's place (and the DICTID of the zlib wrapper is worked out)
    const uint8_t* dm = c->meta.as<uint8_t>();
    const uint64_t* d_joff = (const uint64_t*)(dm + ml.joff);
    MARK("start");
    // DICTID (zlib): the adler32 of each distinct dictionary, once
    if (req.wrap == 1)
      zs_k_checksum<<<p.ndict, 64, 0, st>>>(dict->d_dict, (const uint64_t*)(dm + ml.uoff),
                                            (const uint32_t*)(dm + ml.ulen), c->dadler.as<uint32_t>(), 1);
    zs_k_dict_join<<<dim3(p.g_join_x, n), 256, 0, st>>>(
        b.in, b.in_off, b.in_len, dict->d_dict, (const uint64_t*)(dm + ml.doff), (const uint32_t*)(dm + ml.dlen),
        (const uint32_t*)(dm + ml.start), c->djoin.as<uint8_t>(), d_joff);
    MARK("dict_join");
    HIPCHK(hipGetLastError());
    const Batch bj = {n, c->djoin.as<uint8_t>(), d_joff, (const uint32_t*)(dm + ml.jlen), b.out, b.out_off, b.out_cap};
    r = deflate_launch(c, st, p, bj, b, d_status, d_out_len, ck, ml.bytes);
  } else {
    r = deflate_launch(c, st, p, b, b, d_status, d_out_len, ck, ml.bytes);
  }
  if (r != ZS_OK) return r;
  return deflate_finish(c, st, p, n, d_status, d_check);
}

// A batch with Z_FULL_FLUSH points (validated; levels 1..9): the plan runs over the SEGMENTS -- the
// pieces between the flush points, each a stream of its own to the match, parse, trees and emit
// kernels -- and the flushed layout joins them per stream (deflate_flush.hip).
// A primed batch (req.primed) is the same batch with each segment widened to its J: lp bytes of
// prime in front (zs_plan_primed), planned as a dictionary of that length, parsed from lp on.
static int deflate_batch_flush(zs_ctx* c, const zs_deflate_req& req, const Batch& h, int32_t* d_status,
                               uint32_t* d_out_len, uint32_t* d_check, hipStream_t st, const FlushIn& flush) {
  const uint32_t n = h.n;
  zs_flush_plan& f = c->fp;
  zs_plan_flush(n, h.in_len, flush.first, flush.pos, f);
  if (req.primed) zs_plan_primed(f);
  const uint32_t M = f.M;
  zs_deflate_plan& p = c->dp;
  zs_plan_deflate(req, c->o, c->fast_group, c->lane_order, M, f.slen.data(), req.primed ? f.lp.data() : nullptr, 0, p);
  const zs_meta_layout& ml = p.ml;
  const zs_flush_layout fo(ml.bytes, n, M);
  HIPCHK(c->check.ensure(4ull * n));
  // the streams' check values' part map behind the flushed section (a raw batch has none)
  const zs_checksum_plan* ck;
  size_t ck_bytes;
  if (const int rc = ck_prepare(c, req.wrap != 0, n, h.in_len, &ck, &ck_bytes)) return rc;
  if (const int rc = deflate_ensure(c, p)) return rc;
  HIPCHK(c->fstreams.ensure(sizeof(zs_stream) * (size_t)n));
  // this batch's scan behind those of the call's chunks before it (deflate_host sized fscan for all)
  zs_ctx::Call& k = c->call;
  k.fscan_at = k.fscan_used;
  HIPCHK(c->fscan.ensure(8ull * k.fscan_at + fo.scan_bytes));
  k.fscan_used += fo.scan_bytes / 8;
  k.fidx.push_back({k.fscan_at, n, M, req.wrap == 1 ? 2u : req.wrap == 2 ? 10u : 0u, f.sfirst});
  // the segments as a batch: their bytes where they lie in their streams, every one with its stream's output
  std::vector<uint64_t> sin(M), sout(M);
  for (uint32_t g = 0; g < M; g++) {
    sin[g] = h.in_off[f.sstream[g]] + (req.primed ? f.joff[g] : f.soff[g]);
    sout[g] = h.out_off[f.sstream[g]];
  }
  const Batch hs = {M, h.in, sin.data(), req.primed ? f.nv.data() : f.slen.data(), h.out, sout.data(), nullptr};
  Batch b;
  const int r = upload_batch(c, st, ml, fo.bytes + ck_bytes, hs, &b, [&](uint8_t* hm) {
    ck_fill(ck, hm + fo.bytes);
    if (req.primed) memcpy(hm + ml.start, p.start.data(), 4ull * M);
    memcpy(hm + ml.pos_base, p.pos.data(), 8ull * M);
    memcpy(hm + ml.blk_base, p.blk.data(), 4ull * M);
    if (!p.segs.empty()) memcpy(hm + ml.segs, p.segs.data(), sizeof(zs_sweep_seg) * p.segs.size());
    memcpy(hm + fo.in_off, h.in_off, 8ull * n);
    memcpy(hm + fo.in_len, h.in_len, 4ull * n);
    memcpy(hm + fo.out_off, h.out_off, 8ull * n);
    memcpy(hm + fo.out_cap, h.out_cap, 4ull * n);
    memcpy(hm + fo.sfirst, f.sfirst.data(), 4ull * (n + 1));
    memcpy(hm + fo.sstream, f.sstream.data(), 4ull * (M + 1));
  });
  if (r != ZS_OK) return r;
  const uint8_t* dm = c->meta.as<uint8_t>();
  const Batch real = {n, h.in, (const uint64_t*)(dm + fo.in_off), (const uint32_t*)(dm + fo.in_len), h.out,
                      (const uint64_t*)(dm + fo.out_off), (const uint32_t*)(dm + fo.out_cap)};
  const FlushDev fd = {(const uint32_t*)(dm + fo.sfirst), (const uint32_t*)(dm + fo.sstream)};
  const int rl = deflate_launch(c, st, p, b, real, d_status, d_out_len, ck, fo.bytes, &fd);
  if (rl != ZS_OK) return rl;
  return deflate_finish(c, st, p, n, d_status, d_check);
}

// A BGZF batch (validated): the plan runs over the SEGMENTS -- the pieces of req.bgzf bytes, each
// a finished raw stream to the match, parse, trees and emit kernels -- and the BGZF layout frames them per
// stream (deflate_bgzf.hip).  Level 0 plans no parse: zs_k_bgzf_stored writes the members from the maps alone.
static int deflate_batch_bgzf(zs_ctx* c, const zs_deflate_req& req, const Batch& h, int32_t* d_status,
                              uint32_t* d_out_len, uint32_t* d_check, hipStream_t st) {
  const uint32_t n = h.n;
  zs_flush_plan& f = c->fp;
  zs_plan_bgzf(n, h.in_len, req.bgzf, f);
  const uint32_t M = f.M;
  zs_deflate_plan& p = c->dp;
  zs_plan_deflate(req, c->o, c->fast_group, c->lane_order, M, f.slen.data(), nullptr, 0, p);
  const zs_meta_layout& ml = p.ml;
  const zs_flush_layout fo(ml.bytes, n, M);
  HIPCHK(c->check.ensure(4ull * ((size_t)n + M)));  // the streams' crc32, then the members'
  const zs_checksum_plan* ck;
  size_t ck_bytes;
  if (const int rc = ck_prepare(c, true, n, h.in_len, &ck, &ck_bytes)) return rc;
  if (const int rc = deflate_ensure(c, p)) return rc;
  zs_ctx::Call& k = c->call;
  zs_ctx::FlushIdx idx = {0, n, M, 0, f.sfirst};
  idx.bgzf = true;
  idx.soff = f.soff;
  idx.in_len.assign(h.in_len, h.in_len + n);
  if (p.stored) {
    idx.stored_member = req.bgzf + ZS_BGZF_HEADER + 5 + ZS_BGZF_TRAILER;
  } else {
    HIPCHK(c->fstreams.ensure(sizeof(zs_stream) * (size_t)n));
    // this batch's scan behind those of the call's chunks before it (deflate_host sized fscan for all)
    k.fscan_at = k.fscan_used;
    HIPCHK(c->fscan.ensure(8ull * k.fscan_at + fo.scan_bytes));
    k.fscan_used += fo.scan_bytes / 8;
    idx.at = k.fscan_at;
  }
  k.fidx.push_back(std::move(idx));
  // the segments as a batch: their bytes where they lie in their streams, every one with its stream's output
  std::vector<uint64_t> sin(M + 1), sout(M + 1);
  std::vector<uint32_t> slen(M + 1);
  for (uint32_t g = 0; g < M; g++) {
    sin[g] = h.in_off[f.sstream[g]] + f.soff[g];
    sout[g] = h.out_off[f.sstream[g]];
    slen[g] = f.slen[g];
  }
  const Batch hs = {M, h.in, sin.data(), slen.data(), h.out, sout.data(), nullptr};
  Batch b;
  const int r = upload_batch(c, st, ml, fo.bytes + ck_bytes, hs, &b, [&](uint8_t* hm) {
    ck_fill(ck, hm + fo.bytes);
    if (!p.stored && M) {
      memcpy(hm + ml.pos_base, p.pos.data(), 8ull * M);
      memcpy(hm + ml.blk_base, p.blk.data(), 4ull * M);
      if (!p.segs.empty()) memcpy(hm + ml.segs, p.segs.data(), sizeof(zs_sweep_seg) * p.segs.size());
    }
    memcpy(hm + fo.in_off, h.in_off, 8ull * n);
    memcpy(hm + fo.in_len, h.in_len, 4ull * n);
    memcpy(hm + fo.out_off, h.out_off, 8ull * n);
    memcpy(hm + fo.out_cap, h.out_cap, 4ull * n);
    memcpy(hm + fo.sfirst, f.sfirst.data(), 4ull * (n + 1));
    memcpy(hm + fo.sstream, f.sstream.data(), 4ull * (M + 1));
  });
  if (r != ZS_OK) return r;
  const uint8_t* dm = c->meta.as<uint8_t>();
  const Batch real = {n, h.in, (const uint64_t*)(dm + fo.in_off), (const uint32_t*)(dm + fo.in_len), h.out,
                      (const uint64_t*)(dm + fo.out_off), (const uint32_t*)(dm + fo.out_cap)};
  const FlushDev fd = {(const uint32_t*)(dm + fo.sfirst), (const uint32_t*)(dm + fo.sstream), req.bgzf};
  const int rl = deflate_launch(c, st, p, b, real, d_status, d_out_len, ck, fo.bytes, &fd);
  if (rl != ZS_OK) return rl;
  return deflate_finish(c, st, p, n, d_status, d_check);
}

// The shared body of the public device entries: the call begins once it is neither refused nor empty.
static int deflate_device(zs_ctx* c, const zs_deflate_req& req, const Batch& h, int32_t* d_status, uint32_t* d_out_len,
                          uint32_t* d_check, void* hip_stream, const DictIn* dict, const FlushIn* flush = nullptr) {
  if (!c) return fail(ZS_STREAM_ERROR, "null context");
  const zs_deflate_call a = deflate_call(h, true, dict, flush);
  if (const zs_deflate_err e = zs_deflate_validate(req, c->o, a)) return deflate_fail(e);
  HIPCHK(hipSetDevice(c->device));
  if (h.n == 0) return ZS_OK;
  call_begin(c, CALL_DEFLATE);
  return deflate_batch(c, req, a, h, d_status, d_out_len, d_check, hip_stream ? (hipStream_t)hip_stream : c->stream, dict,
                       flush);
}

extern "C" int zs_deflate_batch_device_ex(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* d_in,
                                          const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                          const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                          uint32_t* d_out_len, uint32_t* d_check, void* hip_stream) {
  zs_deflate_req req;
  zs_deflate_make_req(level, wbits, ZS_STRAT_DEFAULT, false, &req);
  return deflate_device(c, req, {n, d_in, in_off, in_len, d_out, out_off, out_cap}, d_status, d_out_len, d_check,
                        hip_stream, nullptr);
}

extern "C" int zs_deflate_batch_device(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* d_in,
                                       const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                       const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                       uint32_t* d_out_len, void* hip_stream) {
  return zs_deflate_batch_device_ex(c, level, wbits, n, d_in, in_off, in_len, d_out, out_off, out_cap, d_status,
                                    d_out_len, nullptr, hip_stream);
}

// ---------------------------------------------------------- host buffers
// The host-buffer entry points: the caller's streams are packed (in parallel)
// into a pinned staging buffer and copied to HBM; after the batch the outputs
// are compacted on the device (4-aligned, in stream order) and come back in one
// copy of exactly the produced bytes, which the host then scatters to the
// caller's offsets -- chunk by chunk, overlapped with the kernels (host_batch).
static void par_copy(uint32_t n, uint8_t* dst, const uint64_t* dst_off, const uint8_t* src, const uint64_t* src_off,
                     const uint32_t* len, uint64_t total) {
  const int T = total >= (32u << 20) ? 8 : (total >= (4u << 20) ? 4 : 1);
  auto part = [&](int t) {
    for (uint32_t i = (uint32_t)t; i < n; i += (uint32_t)T)
      if (len[i]) memcpy(dst + dst_off[i], src + src_off[i], len[i]);
  };
  if (T == 1) { part(0); return; }
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++) th.emplace_back(part, t);
  for (auto& x : th) x.join();
}

static int stage_in(zs_ctx* c, uint32_t n, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                    std::vector<uint64_t>& doff, uint64_t& total) {
  total = 0;
  doff.resize(n);
  for (uint32_t i = 0; i < n; i++) { doff[i] = total; total += in_len[i]; }
  HIPCHK(c->d_in.ensure(total + 16));
  HIPCHK(c->h_in.ensure(total + 16));
  par_copy(n, c->h_in.as<uint8_t>(), doff.data(), in, in_off, in_len, total);
  if (total) HIPCHK(hipMemcpyAsync(c->d_in.p, c->h_in.p, total, hipMemcpyHostToDevice, c->stream));
  return ZS_OK;
}

// dst[poff[s] ...] = src[soff[s] ...], len[s] bytes (all offsets multiples of 4)
__global__ void zs_k_compact(const uint8_t* __restrict__ src, const uint64_t* __restrict__ offs,
                             const uint32_t* __restrict__ len, uint8_t* __restrict__ dst, uint32_t n) {
  const uint32_t s = blockIdx.x;
  if (s >= n) return;
  const uint32_t words = (len[s] + 3) / 4;
  const uint32_t* a = (const uint32_t*)(src + offs[s]);
  uint32_t* b = (uint32_t*)(dst + offs[n + s]);
  for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) b[i] = a[i];
}

// The host-buffer entries, pipelined: the batch runs as a few chunks of
// streams ([1/8, 3/8, 3/8, 1/8] of them for batches of 32 MB or more: zs_plan_host_chunks), so that
// packing chunk k+1 into the pinned staging and its H2D copy (stream h2d) run
// while chunk k's kernels do (the context's stream), and chunk k-1's output
// compaction, D2H copy (stream d2h) and scatter into the caller's buffers run
// while chunk k+1's do.  h: the caller's batch, host memory; its regions on the device are the
// capacities rounded up to whole words (zs_host_region_cap: the kernels store dwords), the exact
// capacities stay the Z_BUF_ERROR limits.  `launch(a, b, doff, ooff, d_res)` enqueues the
// device batch of streams [a, b) on c->stream; d_res holds nres u32 arrays of n
// entries (array r at d_res + r n), res_host the caller's nres arrays, of which
// res_host[len_idx] is the output length.  Outputs land at h.out + h.out_off[i].
template <class Launch>
static int host_batch_run(zs_ctx* c, const Batch& h, uint32_t nres, uint32_t* const* res_host, uint32_t len_idx,
                          Launch launch, bool one_chunk) {
  const uint32_t n = h.n;
  std::vector<uint64_t> doff(n), ooff(n);
  std::vector<uint32_t> ocap(n);
  uint64_t tin = 0, tout = 0;
  for (uint32_t i = 0; i < n; i++) {
    ocap[i] = zs_host_region_cap(h.out_cap[i]);
    doff[i] = tin;
    tin += h.in_len[i];
    ooff[i] = tout;
    tout += ocap[i];
  }
  HIPCHK(c->d_in.ensure(tin + 16));
  HIPCHK(c->h_in.ensure(tin + 16));
  HIPCHK(c->d_out.ensure(tout + 16));
  // the packed outputs (d_pack, h_out) hold produced bytes, not capacities: a
  // first guess, grown in after_kernels once the chunks before are scattered
  const uint64_t pack0 = zs_plan_host_pack0(c->o, tin, tout);
  HIPCHK(c->d_pack.ensure(pack0));
  HIPCHK(c->h_out.ensure(pack0));
  HIPCHK(c->d_res.ensure(4ull * nres * n + 16));
  HIPCHK(c->h_res.ensure(4ull * nres * n + 16));
  HIPCHK(c->d_offs.ensure(16ull * n + 16));
  HIPCHK(c->h_offs.ensure(16ull * n + 16));
  std::vector<uint32_t> bnd;
  zs_plan_host_chunks(c->o, n, tin, bnd);
  if (one_chunk) bnd = {0u, n};  // (a call that finds its restart points: its scan is not chunked)
  const uint32_t K = (uint32_t)bnd.size() - 1;
  while (c->hev.size() < 3 * K) {
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->hev.push_back(e);
  }
  hipEvent_t* ev_in = c->hev.data();
  hipEvent_t* ev_k = ev_in + K;
  hipEvent_t* ev_out = ev_k + K;
  uint8_t* hin = c->h_in.as<uint8_t>();
  uint32_t* dres = c->d_res.as<uint32_t>();
  uint32_t* hres = c->h_res.as<uint32_t>();
  uint64_t* hoffs = c->h_offs.as<uint64_t>();
  std::vector<uint64_t> poff(n);
  std::vector<char> scattered(K, 0);
  uint64_t packed = 0;  // bytes of the pack buffers in use (chunks not yet scattered)
  // chunk k's bytes are in pinned memory: into the caller's buffers
  auto after_copy = [&](uint32_t k) -> int {
    if (scattered[k]) return ZS_OK;
    const uint32_t a = bnd[k], b = bnd[k + 1];
    HIPCHK(hipEventSynchronize(ev_out[k]));
    uint64_t bytes = 0;
    for (uint32_t i = a; i < b; i++) bytes += res_host[len_idx][i];
    par_copy(b - a, h.out, h.out_off + a, c->h_out.as<uint8_t>(), poff.data() + a, res_host[len_idx] + a, bytes);
    scattered[k] = 1;
    return ZS_OK;
  };
  // chunk k's results are in: the caller's arrays, then its compaction and D2H (stream d2h)
  auto after_kernels = [&](uint32_t k) -> int {
    const uint32_t a = bnd[k], b = bnd[k + 1], m = b - a;
    HIPCHK(hipEventSynchronize(ev_k[k]));
    for (uint32_t r = 0; r < nres; r++)
      if (res_host[r]) memcpy(res_host[r] + a, hres + (size_t)r * n + a, 4ull * m);
    const uint32_t* len = res_host[len_idx];
    uint64_t Pk = 0;
    for (uint32_t i = a; i < b; i++) {
      if (len[i] > ocap[i])
        return fail(ZS_MEM_ERROR, "stream %s reported more output than its capacity", std::to_string(i).c_str());
      Pk += ((uint64_t)len[i] + 3) & ~3ull;
    }
    if (packed + Pk + 16 > std::min(c->d_pack.cap, c->h_out.cap)) {
      // the pack buffers are full: scatter the chunks still in them, then start over (grown)
      for (uint32_t j = 0; j < k; j++) {
        const int rc = after_copy(j);
        if (rc != ZS_OK) return rc;
      }
      packed = 0;
      HIPCHK(c->d_pack.ensure(Pk + 16));
      HIPCHK(c->h_out.ensure(Pk + 16));
    }
    uint64_t P = packed;
    for (uint32_t i = a; i < b; i++) {
      hoffs[2 * a + (i - a)] = ooff[i];
      hoffs[2 * a + m + (i - a)] = poff[i] = P;
      P += ((uint64_t)len[i] + 3) & ~3ull;
    }
    if (P > packed) {
      uint64_t* doffs = c->d_offs.as<uint64_t>() + 2 * a;
      HIPCHK(hipMemcpyAsync(doffs, hoffs + 2 * a, 16ull * m, hipMemcpyHostToDevice, c->d2h));
      zs_k_compact<<<m, 256, 0, c->d2h>>>(c->d_out.as<uint8_t>(), doffs, dres + (size_t)len_idx * n + a,
                                          c->d_pack.as<uint8_t>(), m);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(c->h_out.as<uint8_t>() + packed, c->d_pack.as<uint8_t>() + packed, P - packed,
                            hipMemcpyDeviceToHost, c->d2h));
    }
    packed = P;
    HIPCHK(hipEventRecord(ev_out[k], c->d2h));
    return ZS_OK;
  };
  for (uint32_t k = 0; k < K; k++) {
    const uint32_t a = bnd[k], b = bnd[k + 1], m = b - a;
    const uint64_t bytes = (b < n ? doff[b] : tin) - doff[a];
    par_copy(m, hin, doff.data() + a, h.in, h.in_off + a, h.in_len + a, bytes);
    if (bytes) HIPCHK(hipMemcpyAsync(c->d_in.as<uint8_t>() + doff[a], hin + doff[a], bytes, hipMemcpyHostToDevice, c->h2d));
    HIPCHK(hipEventRecord(ev_in[k], c->h2d));
    HIPCHK(hipStreamWaitEvent(c->stream, ev_in[k], 0));
    std::vector<uint32_t*> dr(nres);
    for (uint32_t r = 0; r < nres; r++) dr[r] = dres + (size_t)r * n + a;
    int rc = launch(a, b, doff.data() + a, ooff.data() + a, dr.data());
    if (rc != ZS_OK) return rc;
    c->call.host_chunks = K;
    for (uint32_t r = 0; r < nres; r++)
      HIPCHK(hipMemcpyAsync(hres + (size_t)r * n + a, dr[r], 4ull * m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(ev_k[k], c->stream));
    if (k >= 1 && (rc = after_kernels(k - 1)) != ZS_OK) return rc;
    if (k >= 2 && (rc = after_copy(k - 2)) != ZS_OK) return rc;
  }
  int rc = after_kernels(K - 1);
  if (rc == ZS_OK && K >= 2) rc = after_copy(K - 2);
  if (rc == ZS_OK) rc = after_copy(K - 1);
  return rc;
}

// host_batch_run, and on any error the copies and kernels it left in flight
// are waited for before returning (the next call reuses the staging buffers)
template <class Launch>
static int host_batch(zs_ctx* c, const Batch& h, uint32_t nres, uint32_t* const* res_host, uint32_t len_idx,
                      Launch launch, bool one_chunk = false) {
  const int rc = host_batch_run(c, h, nres, res_host, len_idx, launch, one_chunk);
  if (rc != ZS_OK) {
    (void)hipStreamSynchronize(c->h2d);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->d2h);
  }
  return rc;
}

// The distinct dictionaries of a host call, packed, to the device once (the chunks share them); poff: the
// members' dictionaries' offsets in c->d_dict
static int host_dict_upload(zs_ctx* c, uint32_t n, const DictIn& dict, std::vector<uint64_t>& poff) {
  zs_dict_set ds;
  std::vector<uint64_t> upos;
  zs_dict_distinct(n, dict.off, dict.len, ds);
  const uint64_t dbytes = zs_dict_pack_layout(ds, n, dict.len, upos, poff);
  HIPCHK(c->d_dict.ensure(dbytes + 16));
  if (!dbytes) return ZS_OK;
  std::vector<uint8_t> pack(dbytes);
  zs_dict_pack(ds, upos, dict.d_dict, pack.data());
  HIPCHK(hipMemcpy(c->d_dict.p, pack.data(), dbytes, hipMemcpyHostToDevice));
  return ZS_OK;
}

// The host compress of every zs_deflate_batch* entry.  dict (requests with req.dict, else null):
// the caller's dictionary bytes, offsets and lengths, all host memory.
// h: the caller's batch, host memory too.
static int deflate_host(zs_ctx* c, const zs_deflate_req& req, const Batch& h, int32_t* status, uint32_t* out_len,
                        uint32_t* check, const DictIn* dict, const FlushIn* flush = nullptr) {
  if (!c) return fail(ZS_STREAM_ERROR, "null context");
  const uint32_t n = h.n;
  const zs_deflate_call call = deflate_call(h, false, dict, flush);
  if (const zs_deflate_err e = zs_deflate_validate_host(req, call)) return deflate_fail(e);
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return ZS_OK;
  // the request's own faults (windowBits, level, strategy), which the first chunk would name next: here, so
  // that a call refused for them has not begun
  if (const zs_deflate_err e = zs_deflate_validate(req, c->o, zs_deflate_call())) return deflate_fail(e);
  // a batch without any dictionary is the plain batch
  zs_deflate_req rq = req;
  rq.dict = zs_deflate_any_dict(req, call);
  std::vector<uint64_t> poff;
  if (rq.dict)
    if (const int r = host_dict_upload(c, n, *dict, poff)) return r;
  // a flushed batch: room for the scans of all its chunks, so that none is lost to a regrown buffer
  // before zs_last_flush_index reads them
  if (zs_deflate_any_flush(rq, call)) {
    const uint64_t mt = (uint64_t)n + (flush->first[n] - flush->first[0]);
    HIPCHK(c->fscan.ensure(8ull * (mt + mt / ZS_FLUSH_TILE + 16)));
  }
  if (rq.bgzf) {  // ... and a BGZF batch's, before zs_last_bgzf_blocks reads them
    uint64_t mt = n;
    for (uint32_t i = 0; i < n; i++) mt += zs_bgzf_blocks(h.in_len[i], rq.bgzf);
    HIPCHK(c->fscan.ensure(8ull * (mt + mt / ZS_FLUSH_TILE + 16)));
  }
  call_begin(c, CALL_DEFLATE);
  uint32_t* res[3] = {(uint32_t*)status, out_len, check};
  return host_batch(c, h, 3, res, 1,
                    [&](uint32_t a, uint32_t b, const uint64_t* doff, const uint64_t* ooff, uint32_t** dr) {
                      const DictIn di = rq.dict ? DictIn{c->d_dict.as<uint8_t>(), poff.data() + a, dict->len + a} : DictIn{};
                      // (a chunk's positions: the same position array, the chunk's part of the index)
                      const FlushIn fi = flush ? FlushIn{flush->first + a, flush->pos} : FlushIn{};
                      const Batch hb = {b - a, c->d_in.as<uint8_t>(), doff, h.in_len + a, c->d_out.as<uint8_t>(), ooff,
                                        h.out_cap + a};
                      const DictIn* cd = rq.dict ? &di : nullptr;
                      const FlushIn* cf = flush ? &fi : nullptr;
                      const zs_deflate_call ca = deflate_call(hb, false, cd, cf);
                      if (const zs_deflate_err e = zs_deflate_validate(rq, c->o, ca)) return deflate_fail(e);
                      return deflate_batch(c, rq, ca, hb, (int32_t*)dr[0], dr[1], check ? dr[2] : nullptr, c->stream, cd,
                                           cf);
                    });  // out_len is 0 for failed streams
}

extern "C" int zs_deflate_batch_ex(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* in,
                                   const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                   const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                   uint32_t* out_len, uint32_t* check) {
  zs_deflate_req req;
  zs_deflate_make_req(level, wbits, ZS_STRAT_DEFAULT, false, &req);
  return deflate_host(c, req, {n, in, in_off, in_len, out, out_off, out_cap}, status, out_len, check, nullptr);
}

extern "C" int zs_deflate_batch(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                const uint32_t* in_len, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                int32_t* status, uint32_t* out_len) {
  return zs_deflate_batch_ex(c, level, wbits, n, in, in_off, in_len, out, out_off, out_cap, status, out_len, nullptr);
}

// ---- Z_FULL_FLUSH points (deflate()'s flush argument, deflate.ts:716-989; the flush branch :942-961): a
// fault of `flush` is reported before the context is looked at
extern "C" uint64_t zs_deflate_bound_flush(uint64_t source_len, int wbits, uint64_t n_flush) {
  // every extra piece costs at most the raw bound's constant 7 and the marker's 5 bytes
  return zs_deflate_bound(source_len, wbits) + 12 * n_flush;
}

extern "C" int zs_deflate_batch_flush_device(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* d_in,
                                             const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                             const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                             uint32_t* d_out_len, uint32_t* d_check, void* hip_stream, int flush,
                                             const uint64_t* flush_first, const uint32_t* flush_pos) {
  zs_deflate_req req;
  if (const zs_deflate_err e = zs_deflate_make_req_flush(level, wbits, flush, &req)) return deflate_fail(e);
  const FlushIn fi = {flush_first, flush_pos};
  return deflate_device(c, req, {n, d_in, in_off, in_len, d_out, out_off, out_cap}, d_status, d_out_len, d_check,
                        hip_stream, nullptr, &fi);
}

extern "C" int zs_deflate_batch_flush(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* in,
                                      const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                      const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                      uint32_t* out_len, uint32_t* check, int flush, const uint64_t* flush_first,
                                      const uint32_t* flush_pos) {
  zs_deflate_req req;
  if (const zs_deflate_err e = zs_deflate_make_req_flush(level, wbits, flush, &req)) return deflate_fail(e);
  const FlushIn fi = {flush_first, flush_pos};
  return deflate_host(c, req, {n, in, in_off, in_len, out, out_off, out_cap}, status, out_len, check, nullptr, &fi);
}

// ---- primed pieces: the _flush entries without `flush`
extern "C" int zs_deflate_batch_primed_device(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* d_in,
                                              const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                              const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                              uint32_t* d_out_len, uint32_t* d_check, void* hip_stream,
                                              const uint64_t* flush_first, const uint32_t* flush_pos) {
  zs_deflate_req req;
  zs_deflate_make_req_primed(level, wbits, &req);
  const FlushIn fi = {flush_first, flush_pos};
  return deflate_device(c, req, {n, d_in, in_off, in_len, d_out, out_off, out_cap}, d_status, d_out_len, d_check,
                        hip_stream, nullptr, &fi);
}

extern "C" int zs_deflate_batch_primed(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* in,
                                       const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                       const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                       uint32_t* out_len, uint32_t* check, const uint64_t* flush_first,
                                       const uint32_t* flush_pos) {
  zs_deflate_req req;
  zs_deflate_make_req_primed(level, wbits, &req);
  const FlushIn fi = {flush_first, flush_pos};
  return deflate_host(c, req, {n, in, in_off, in_len, out, out_off, out_cap}, status, out_len, check, nullptr, &fi);
}

// ---- BGZF (SAM specification 4.1): the level's, the block size's, the arrays' and the count's
// faults are reported before the context is looked at, in that order
extern "C" uint64_t zs_deflate_bound_bgzf(uint64_t source_len, uint32_t block_bytes) {
  return zs_bgzf_bound(source_len, block_bytes);
}

// device: the streams + blocks of the one device call are counted; a host call's chunks count their own
static int bgzf_req(int level, uint32_t block_bytes, const Batch& h, bool device, zs_deflate_req* req) {
  if (const zs_deflate_err e = zs_deflate_make_req_bgzf(level, block_bytes, req)) return deflate_fail(e);
  zs_deflate_call a;
  a.n = h.n;
  a.in_len = h.in_len;
  a.null_arrays = h.n && (!h.in_off || !h.in_len || !h.out_off || !h.out_cap);
  if (const zs_deflate_err e = zs_deflate_validate_bgzf(*req, a, device)) return deflate_fail(e);
  return ZS_OK;
}

extern "C" int zs_deflate_batch_bgzf_device(zs_ctx* c, int level, uint32_t n, const uint8_t* d_in, const uint64_t* in_off,
                                            const uint32_t* in_len, uint8_t* d_out, const uint64_t* out_off,
                                            const uint32_t* out_cap, int32_t* d_status, uint32_t* d_out_len,
                                            uint32_t* d_check, void* hip_stream, uint32_t block_bytes) {
  const Batch h = {n, d_in, in_off, in_len, d_out, out_off, out_cap};
  zs_deflate_req req;
  if (const int r = bgzf_req(level, block_bytes, h, true, &req)) return r;
  return deflate_device(c, req, h, d_status, d_out_len, d_check, hip_stream, nullptr);
}

extern "C" int zs_deflate_batch_bgzf(zs_ctx* c, int level, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                     const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                     const uint32_t* out_cap, int32_t* status, uint32_t* out_len, uint32_t* check,
                                     uint32_t block_bytes) {
  const Batch h = {n, in, in_off, in_len, out, out_off, out_cap};
  zs_deflate_req req;
  if (const int r = bgzf_req(level, block_bytes, h, false, &req)) return r;
  return deflate_host(c, req, h, status, out_len, check, nullptr);
}

// The blocks of the last BGZF compress call on the context, in the layout of zs_last_members: block_first
// (n + 1 entries, from 0), then at most `cap` blocks' (offset of the block's first input byte, offset of
// its first byte in the stream's output), every stream's end-of-file block included: (in_len, out_len - 28).
// The output offsets are the layout's scan (zs_k_bgzf_local's, which zs_k_bgzf_place rebases the blocks
// by); a host entry's chunks follow each other.  A stream that failed has the offsets it would have had.
extern "C" uint64_t zs_last_bgzf_blocks(zs_ctx* c, uint64_t* block_first, uint32_t* block_in, uint32_t* block_out,
                                        uint64_t cap) {
  if (!c || c->call.fidx.empty() || !c->call.fidx[0].bgzf) return 0;
  std::vector<uint64_t> scan(c->call.fscan_used);
  if (!scan.empty()) {
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 0;
    if (hipMemcpy(scan.data(), c->fscan.p, 8ull * scan.size(), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  }
  uint64_t k = 0, s_all = 0;
  auto put = [&](uint32_t in_pos, uint64_t out_pos) {
    if (k < cap) {
      if (block_in) block_in[k] = in_pos;
      if (block_out) block_out[k] = (uint32_t)out_pos;
    }
    k++;
  };
  if (block_first) block_first[0] = 0;
  for (const zs_ctx::FlushIdx& f : c->call.fidx) {
    const uint64_t* segx = f.stored_member ? nullptr : scan.data() + f.at;
    const uint64_t* tile = f.stored_member ? nullptr : segx + f.M + 1;
    // the bytes of all members before x
    auto at = [&](uint32_t x) { return segx ? tile[x / ZS_FLUSH_TILE] + segx[x] : 0; };
    for (uint32_t s = 0; s < f.n; s++, s_all++) {
      const uint32_t g0 = f.sfirst[s], g1 = f.sfirst[s + 1];
      for (uint32_t g = g0; g < g1; g++) put(f.soff[g], segx ? at(g) - at(g0) : (uint64_t)(g - g0) * f.stored_member);
      put(f.in_len[s], segx ? at(g1) - at(g0) : f.in_len[s] + (uint64_t)(g1 - g0) * (ZS_BGZF_HEADER + 5 + ZS_BGZF_TRAILER));
      if (block_first) block_first[s_all + 1] = k;
    }
  }
  return k;
}

// ---- compression strategies (deflateInit2_'s strategy: validation deflate.ts:289-290, dispatch :923-931)
extern "C" int zs_deflate_batch_strategy_device(zs_ctx* c, int level, int strategy, int wbits, uint32_t n,
                                                const uint8_t* d_in, const uint64_t* in_off, const uint32_t* in_len,
                                                uint8_t* d_out, const uint64_t* out_off, const uint32_t* out_cap,
                                                int32_t* d_status, uint32_t* d_out_len, uint32_t* d_check,
                                                void* hip_stream) {
  zs_deflate_req req;
  if (const zs_deflate_err e = zs_deflate_make_req(level, wbits, strategy, false, &req)) return deflate_fail(e);
  return deflate_device(c, req, {n, d_in, in_off, in_len, d_out, out_off, out_cap}, d_status, d_out_len, d_check,
                        hip_stream, nullptr);
}

extern "C" int zs_deflate_batch_strategy(zs_ctx* c, int level, int strategy, int wbits, uint32_t n, const uint8_t* in,
                                         const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                         const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                         uint32_t* out_len, uint32_t* check) {
  zs_deflate_req req;
  if (const zs_deflate_err e = zs_deflate_make_req(level, wbits, strategy, false, &req)) return deflate_fail(e);
  return deflate_host(c, req, {n, in, in_off, in_len, out, out_off, out_cap}, status, out_len, check, nullptr);
}

// ---- windowBits and memLevel (deflateInit2_, deflate.ts:253-343; validation :281-294): a fault of
// theirs is reported before the context is looked at
extern "C" int zs_deflate_batch_params_device(zs_ctx* c, int level, int wbits, int mem_level, uint32_t n,
                                              const uint8_t* d_in, const uint64_t* in_off, const uint32_t* in_len,
                                              uint8_t* d_out, const uint64_t* out_off, const uint32_t* out_cap,
                                              int32_t* d_status, uint32_t* d_out_len, uint32_t* d_check,
                                              void* hip_stream) {
  zs_deflate_req req;
  if (const zs_deflate_err e = zs_deflate_make_req_params(level, wbits, mem_level, &req)) return deflate_fail(e);
  return deflate_device(c, req, {n, d_in, in_off, in_len, d_out, out_off, out_cap}, d_status, d_out_len, d_check,
                        hip_stream, nullptr);
}

extern "C" int zs_deflate_batch_params(zs_ctx* c, int level, int wbits, int mem_level, uint32_t n, const uint8_t* in,
                                       const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                       const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                       uint32_t* out_len, uint32_t* check) {
  zs_deflate_req req;
  if (const zs_deflate_err e = zs_deflate_make_req_params(level, wbits, mem_level, &req)) return deflate_fail(e);
  return deflate_host(c, req, {n, in, in_off, in_len, out, out_off, out_cap}, status, out_len, check, nullptr);
}

// ---- preset dictionaries (deflateSetDictionary, deflate.ts:367-424; FDICT / DICTID, deflate.ts:767-778)
extern "C" int zs_deflate_batch_dict_device(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* d_in,
                                            const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                            const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                            uint32_t* d_out_len, uint32_t* d_check, void* hip_stream,
                                            const uint8_t* d_dict, const uint64_t* dict_off,
                                            const uint32_t* dict_len) {
  zs_deflate_req req;
  zs_deflate_make_req(level, wbits, ZS_STRAT_DEFAULT, true, &req);
  const DictIn di = {d_dict, dict_off, dict_len};
  return deflate_device(c, req, {n, d_in, in_off, in_len, d_out, out_off, out_cap}, d_status, d_out_len, d_check,
                        hip_stream, &di);
}

extern "C" int zs_deflate_batch_dict(zs_ctx* c, int level, int wbits, uint32_t n, const uint8_t* in,
                                     const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                     const uint64_t* out_off, const uint32_t* out_cap, int32_t* status,
                                     uint32_t* out_len, uint32_t* check, const uint8_t* dict,
                                     const uint64_t* dict_off, const uint32_t* dict_len) {
  zs_deflate_req req;
  zs_deflate_make_req(level, wbits, ZS_STRAT_DEFAULT, true, &req);
  const DictIn di = {dict, dict_off, dict_len};  // (host memory here)
  return deflate_host(c, req, {n, in, in_off, in_len, out, out_off, out_cap}, status, out_len, check, &di);
}

static int checksum_batch(zs_ctx* c, int kind, uint32_t n, const uint8_t* d_in, const uint64_t* in_off,
                          const uint32_t* in_len, const uint32_t* seeds, uint32_t* d_check, void* hip_stream) {
  if (!c) return fail(ZS_STREAM_ERROR, "null context");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return ZS_OK;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  const zs_meta_layout ml(n);  // (the seeds behind it, then the part map)
  const size_t ck_map = ml.bytes + (seeds ? (4ull * n + 255) & ~size_t(255) : 0);
  call_begin(c, CALL_CHECKSUM);
  const zs_checksum_plan* ck;
  size_t ck_bytes;
  if (const int rc = ck_prepare(c, true, n, in_len, &ck, &ck_bytes)) return rc;
  Batch b;
  const int r = upload_batch(c, st, ml, ck_bytes ? ck_map + ck_bytes : ml.bytes + (seeds ? 4ull * n : 0),
                             {n, d_in, in_off, in_len, nullptr, nullptr, nullptr}, &b, [&](uint8_t* hm) {
                               if (seeds) memcpy(hm + ml.bytes, seeds, 4ull * n);
                               ck_fill(ck, hm + ck_map);
                             });
  if (r != ZS_OK) return r;
  MARK("start");
  ck_launch(c, st, *ck, ck_map, n, b.in, b.in_off, b.in_len, d_check, kind,
            seeds ? (const uint32_t*)(c->meta.as<uint8_t>() + ml.bytes) : nullptr);
  MARK("checksum");
  HIPCHK(hipGetLastError());
  return ZS_OK;  // timing marks are collected when queried (no wait here)
}

extern "C" int zs_crc32_batch_device(zs_ctx* c, uint32_t n, const uint8_t* d_in, const uint64_t* in_off,
                                     const uint32_t* in_len, const uint32_t* seeds, uint32_t* d_check,
                                     void* hip_stream) {
  return checksum_batch(c, 2, n, d_in, in_off, in_len, seeds, d_check, hip_stream);
}
extern "C" int zs_adler32_batch_device(zs_ctx* c, uint32_t n, const uint8_t* d_in, const uint64_t* in_off,
                                       const uint32_t* in_len, const uint32_t* seeds, uint32_t* d_check,
                                       void* hip_stream) {
  return checksum_batch(c, 1, n, d_in, in_off, in_len, seeds, d_check, hip_stream);
}

// host buffers: staged through the context's pinned buffer, results copied back
static int checksum_host(zs_ctx* c, int kind, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                         const uint32_t* in_len, const uint32_t* seeds, uint32_t* check) {
  if (!c) return fail(ZS_STREAM_ERROR, "null context");
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return ZS_OK;
  std::vector<uint64_t> doff;
  uint64_t total = 0;
  int r = stage_in(c, n, in, in_off, in_len, doff, total);
  if (r != ZS_OK) return r;
  HIPCHK(c->d_res.ensure(4ull * n + 16));
  r = checksum_batch(c, kind, n, c->d_in.as<uint8_t>(), doff.data(), in_len, seeds, c->d_res.as<uint32_t>(), nullptr);
  if (r != ZS_OK) return r;
  HIPCHK(hipMemcpyAsync(check, c->d_res.p, 4ull * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return ZS_OK;
}
extern "C" int zs_crc32_batch(zs_ctx* c, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                              const uint32_t* in_len, const uint32_t* seeds, uint32_t* check) {
  return checksum_host(c, 2, n, in, in_off, in_len, seeds, check);
}
extern "C" int zs_adler32_batch(zs_ctx* c, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                const uint32_t* in_len, const uint32_t* seeds, uint32_t* check) {
  return checksum_host(c, 1, n, in, in_off, in_len, seeds, check);
}

// ------------------------------------------------------------------ corpus
namespace {
const char* kVocab =
    "the of and to in is that for it as was with be by on not he this are or his from at which but have an they you "
    "were her she there been one all we their has would when if so no will more can out said up what about its into "
    "them than only other new some could time these two may then do first any my now such like our over man me even "
    "most made after also did many before must through back years where much your way well down should because each "
    "just those people how too little state good very make world still own see men work long get here between both "
    "life being under never day same another know while last might us great old year off come since against go came "
    "right used take three";

struct XS {
  uint32_t s;
  explicit XS(uint32_t seed) : s(seed ? seed : 1) {}
  uint32_t operator()() {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
  }
};

void gen_text(uint32_t seed, uint8_t* out, uint32_t n, const std::vector<std::string>& V) {
  XS r(seed);
  uint32_t o = 0, w = 0;
  while (o < n) {
    const uint32_t a = r();
    const uint32_t idx = std::min(a % 144u, (a >> 12) % 144u);
    const std::string& word = V[idx];
    for (size_t i = 0; i < word.size() && o < n; i++) out[o++] = (uint8_t)word[i];
    if (o < n) out[o++] = (++w % 13 == 0) ? 10 : 32;
  }
}
}  // namespace

extern "C" void zs_corpus(int kind, uint32_t first, uint32_t n_streams, uint32_t len, uint8_t* out, int threads) {
  std::vector<std::string> V;
  {
    std::string all(kVocab), cur;
    for (char ch : all) {
      if (ch == ' ') { V.push_back(cur); cur.clear(); }
      else cur.push_back(ch);
    }
    V.push_back(cur);
  }
  auto one = [&](uint32_t i) {
    const uint32_t seed = 0x9e3779b9u ^ (first + i);
    uint8_t* o = out + (size_t)i * len;
    if (kind == 2) {
      XS r(seed);
      for (uint32_t j = 0; j < len; j++) o[j] = (uint8_t)r();
      return;
    }
    gen_text(seed, o, len, V);
    if (kind == 1) {
      XS r(seed ^ 0x85ebca6bu);
      for (uint32_t k = 0; k + 8192 <= len; k += 8192)
        for (uint32_t j = 0; j < 1024; j++) o[k + 4096 + j] = (uint8_t)r();
    }
  };
  if (threads < 1) threads = 1;
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++)
    th.emplace_back([&, t] {
      for (uint32_t i = (uint32_t)t; i < n_streams; i += (uint32_t)threads) one(i);
    });
  for (auto& x : th) x.join();
}

// ------------------------------------------------------------ introspection
// Copies an intermediate array of stream `s` of the last deflate batch to host
// memory: what = 0 prevd (u16/position, 0xffff = no link), 1 match table (u32x2/position),
// 2 symbols (u32 each; count = streams[s].nsym), 3 blocks (zs_block each),
// 4 stream record (zs_stream), 7 the sweep route's members of the stream's first window
// (u16 each, window-relative: the inserted positions sorted by (hash, position)).
// Returns the number of bytes copied.
extern "C" uint64_t zs_debug_fetch(zs_ctx* c, int what, uint32_t s, void* dst, uint64_t cap) {
  if (c && what >= 16 && what <= 21) {
    // the segmented decode's records of the last inflate batch: 16 counters (-, members
    // finished), 17 spans (zs_seg_blk), 18 lanes (zs_seg_lane), 19 members (zs_seg_mem), 20 found[]
    // (big members), 21 entries (zs_seg_ent)
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    const Buf* b = what == 16 ? &c->gcnt : what == 17 ? &c->gblk : what == 18 ? &c->glanes : what == 19 ? &c->gmem
                   : what == 21 ? &c->gent : &c->gfound;
    const uint64_t bytes = std::min<uint64_t>(cap, b->cap);
    if (!b->p || !bytes || hipMemcpy(dst, b->p, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return bytes;
  }
  if (!c || !c->streams.p) return 0;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)hipDeviceSynchronize();
  zs_stream st;
  if (hipMemcpy(&st, c->streams.as<zs_stream>() + s, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  uint64_t pos_base = 0;
  uint32_t blk_base = 0, n = 0;
  // meta layout of the last call: recompute offsets from the host copy
  const size_t nstreams = c->last_n;
  zs_meta_layout m2((uint32_t)nstreams);
  const uint8_t* hm = c->hmeta.data();
  pos_base = ((const uint64_t*)(hm + m2.pos_base))[s];
  blk_base = ((const uint32_t*)(hm + m2.blk_base))[s];
  n = ((const uint32_t*)(hm + m2.in_len))[s];
  if (s < c->dp.start.size()) n += c->dp.start[s];  // a batch with dictionaries: the joined stream's positions
  const void* src = nullptr;
  uint64_t bytes = 0;
  // (a batch of the tally kernels -- Z_HUFFMAN_ONLY, Z_RLE -- searches no matches: the tables may not be there)
  if ((what == 0 && 2ull * (pos_base + n) > c->prevd.cap) || (what == 1 && 8ull * (pos_base + n) > c->mres.cap)) return 0;
  switch (what) {
    case 0: src = c->prevd.as<uint16_t>() + pos_base; bytes = 2ull * n; break;
    case 1: src = c->mres.as<uint2>() + pos_base; bytes = 8ull * n; break;
    case 2: src = c->syms.as<uint32_t>() + pos_base + s; bytes = 4ull * st.nsym; break;
    case 3: src = c->blocks.as<zs_block>() + blk_base; bytes = sizeof(zs_block) * st.nblk; break;
    case 4: src = c->streams.as<zs_stream>() + s; bytes = sizeof(zs_stream); break;
    case 5: src = c->codes.as<uint32_t>() + (size_t)blk_base * (ZS_L_CODES + ZS_D_CODES); bytes = 4ull * (ZS_L_CODES + ZS_D_CODES) * st.nblk; break;
    case 6: src = c->hdr.as<uint32_t>() + (size_t)blk_base * ZS_HDR_WORDS; bytes = 4ull * ZS_HDR_WORDS * st.nblk; break;
    case 7: {
      const zs_deflate_plan& p = c->dp;
      if (p.match != ZS_MATCH_SWEEP || (size_t)s + 1 >= p.win0.size()) return 0;
      const zs_sweep_seg& g = p.segs[p.win0[s]];
      const uint32_t m = n > 2 ? std::min(n - 2, g.ohi) : 0u;  // zs_k_bucket's member count
      if (2ull * (g.mb + m) > c->prevd.cap) return 0;
      src = c->prevd.as<uint16_t>() + g.mb;
      bytes = 2ull * m;
      break;
    }
    default: return 0;
  }
  bytes = std::min(bytes, cap);
  if (bytes && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return bytes;
}

// ------------------------------------------------------------------ inflate
static const char* kInflateMsgs[ZS_MSG_COUNT] = {
    "",
    "incorrect header check",
    "unknown compression method",
    "invalid window size",
    "unknown header flags set",
    "header crc mismatch",
    "invalid block type",
    "invalid stored block lengths",
    "too many length or distance symbols",
    "too many length",
    "invalid code lengths set",
    "invalid bit length repeat",
    "invalid code -- missing end-of-block",
    "invalid literal/lengths set",
    "invalid distances set",
    "invalid literal/length code",
    "invalid distance code",
    "invalid distance too far back",
    "incorrect data check",
    "incorrect length check",
    "output capacity exceeded",
    "restart points do not decode the stream",
    "",
    "virtual offsets do not follow a chain of BGZF blocks",
};

extern "C" const char* zs_inflate_message(int32_t i) { return (i >= 0 && i < ZS_MSG_COUNT) ? kInflateMsgs[i] : ""; }

__global__ void zs_k_inflate_finish(const zs_inflate_result* r, const zs_lane_res* lane, int32_t* status,
                                    int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed, int n,
                                    uint32_t* lane_count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  if (lane && lane[s].bail == 0) {  // clean member from the lane path
    atomicAdd(lane_count, 1u);
    status[s] = ZS_Z_STREAM_END;
    phase[s] = ZS_PHASE_NONE_;
    msg[s] = ZS_MSG_NONE;
    out_len[s] = lane[s].out_len;
    consumed[s] = lane[s].consumed;
    return;
  }
  status[s] = r[s].status;
  phase[s] = r[s].phase;
  msg[s] = r[s].msg;
  out_len[s] = r[s].out_len;
  consumed[s] = r[s].consumed;
}

// Per-stream check value (the reference's strm.adler after a successful
// stream, inflate.ts:105,1014,1080): the adler32 (zlib) / crc32 (gzip) of the
// output -- equal to the verified trailer, so read from it; 0 for raw and
// deflate64-raw (createStream's initial _adler, common/utils.ts:49, never
// updated without a wrapper) and for a failed stream.
__global__ void zs_k_inflate_check(const uint8_t* in, const uint64_t* in_off, const int32_t* status,
                                   const uint32_t* consumed, int wbits, uint32_t* out, int n) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  uint32_t v = 0;
  if (status[s] == ZS_Z_STREAM_END && wbits > 0) {
    const uint8_t* t = in + in_off[s] + consumed[s] - (wbits == 31 ? 8 : 4);
    v = wbits == 31 ? (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24
                    : (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | (uint32_t)t[3];
  }
  out[s] = v;
}

// The lane kernel's instance for a lane launch of the plan (inflate_lane.hip instantiates these five)
static auto lane_kernel(int rt, bool refw) {
  return refw ? (rt == 2 ? zs_k_inflate_lane<2, true> : zs_k_inflate_lane<0, true>)
              : (rt == 2   ? zs_k_inflate_lane<2, false>
                 : rt == 1 ? zs_k_inflate_lane<1, false>
                           : zs_k_inflate_lane<0, false>);
}
// ... and of a batch with dictionaries: the lane launch over the whole batch
static auto lane_kernel_dict(int rt) {
  return rt == 2 ? zs_k_inflate_lane<2, false, true> : rt == 1 ? zs_k_inflate_lane<1, false, true>
                                                               : zs_k_inflate_lane<0, false, true>;
}

// The segmented decode of the members in c->ip.seg (inflate_seg.hip; h: the batch's
// host arrays, b: its device arrays) on the side stream, after the caller's stream
// reaches this point; then the wave kernel over the same members for any the pieces
// could not finish (skip_done: the others return at once), the exact kernel after
// it for whatever fails there.
static int seg_launch(zs_ctx* c, const zs_route_opts& o, hipStream_t st, int wbits, const Batch& h, const Batch& b,
                      zs_lane_res* lres) {
  const std::vector<uint32_t>& list = c->ip.seg;
  zs_seg_plan& p = c->gp;
  zs_plan_seg(o, wbits, list, h.in_len, h.out_cap, p);
  const uint32_t ng = (uint32_t)list.size(), nb = p.nb, nbig = (uint32_t)p.big.size();
  HIPCHK(c->glist.ensure(4ull * ng));
  HIPCHK(c->gspb.ensure(4ull * (ng + 1)));
  HIPCHK(c->gbig.ensure(4ull * nbig + 4));
  HIPCHK(c->gfound.ensure(8ull * ZS_SPLIT_MAX * nbig + 8));
  HIPCHK(c->gblk.ensure(sizeof(zs_seg_blk) * nb));
  HIPCHK(c->glanes.ensure(sizeof(zs_seg_lane) * ZS_SEG_LANES * nb));
  HIPCHK(c->gtab.ensure(sizeof(zcode) * ZS_SEG_TAB * nb));
  HIPCHK(c->gent.ensure(sizeof(zs_seg_ent) * ZS_SPLIT_MAX * ng));
  HIPCHK(c->gmem.ensure(sizeof(zs_seg_mem) * ng));
  HIPCHK(c->gpbase.ensure(4ull * (ng + 1)));
  HIPCHK(c->gplist.ensure(16ull * p.pbase[ng] + 16));
  HIPCHK(c->gsbase.ensure(8ull * (ng + 1)));
  HIPCHK(c->gscr.ensure(2ull * p.sbase[ng] + 64));
  HIPCHK(c->gcnt.ensure(16));
  // the spans taken (the decode's work list) and the members left over
  HIPCHK(c->gspl.ensure(4ull * nb + 4));
  HIPCHK(c->gflist.ensure(4ull * ng));
  if (nbig) HIPCHK(c->gbigs.ensure(4ull * nbig));
  HIPCHK(hipMemcpyAsync(c->glist.p, list.data(), 4ull * ng, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->gspb.p, p.spb.data(), 4ull * (ng + 1), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->gpbase.p, p.pbase.data(), 4ull * (ng + 1), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->gsbase.p, p.sbase.data(), 8ull * (ng + 1), hipMemcpyHostToDevice, st));
  if (nbig) {
    HIPCHK(hipMemcpyAsync(c->gbigs.p, p.big_s.data(), 4ull * nbig, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->gbig.p, p.big.data(), 4ull * nbig, hipMemcpyHostToDevice, st));
  }
  // fresh records: members (span counters), entries (start 0 = none), spans (member NONE)
  HIPCHK(hipMemsetAsync(c->gmem.p, 0, sizeof(zs_seg_mem) * ng, st));
  HIPCHK(hipMemsetAsync(c->gent.p, 0, sizeof(zs_seg_ent) * ZS_SPLIT_MAX * ng, st));
  HIPCHK(hipMemsetAsync(c->gblk.p, 0xff, sizeof(zs_seg_blk) * nb, st));
  // the counters: spans taken, members left over, and with the call's first segmented launch (a host
  // call's earlier chunks may have had no such member) the members finished
  HIPCHK(hipMemsetAsync(c->gcnt.as<uint32_t>() + 2, 0, 8, st));
  if (!c->call.seg_ran) HIPCHK(hipMemsetAsync(c->gcnt.p, 0, 8, st));
  c->call.seg_ran = true;
  HIPCHK(hipEventRecord(c->fork, st));
  HIPCHK(hipStreamWaitEvent(c->side, c->fork, 0));
  hipStream_t sd = c->side;
  if (int r = mark(c, sd, "start")) return r;
  const uint32_t* gl = c->glist.as<uint32_t>();
  uint64_t* gf = c->gfound.as<uint64_t>();
  uint32_t* cnt = c->gcnt.as<uint32_t>();
  zs_seg_blk* gb = c->gblk.as<zs_seg_blk>();
  zs_seg_lane* gln = c->glanes.as<zs_seg_lane>();
  zcode* gt = c->gtab.as<zcode>();
  zs_seg_ent* ge = c->gent.as<zs_seg_ent>();
  zs_seg_mem* gm = c->gmem.as<zs_seg_mem>();
  const uint32_t* spl = c->gspl.as<uint32_t>();
  const uint64_t* sb = c->gsbase.as<uint64_t>();
  uint16_t* scr = c->gscr.as<uint16_t>();
  uint32_t* llen = c->llen.as<uint32_t>();
  if (nbig) {
    zs_k_split_find<<<nbig * ZS_SPLIT_MAX, 256, 0, sd>>>(b.in, b.in_off, b.in_len, c->gbigs.as<uint32_t>(), wbits, gf);
    if (int r = mark(c, sd, "seg_find")) return r;
  }
  // (large deflate members: the instance whose lanes decode the stretch between their sync windows
  // without the windows' bookkeeping)
  auto walk = p.d64 ? (p.w2k ? zs_k_seg_walk<true, 2048u, false> : zs_k_seg_walk<true, 1024u, false>)
                    : (p.w2k ? zs_k_seg_walk<false, 2048u, true>
                             : p.large ? zs_k_seg_walk<false, 1024u, true> : zs_k_seg_walk<false, 1024u, false>);
  walk<<<p.nwalk, 64, 0, sd>>>(b.in, b.in_off, b.in_len, gl, ng, c->gbig.as<uint32_t>(), nbig, wbits, gf,
                               c->gspb.as<uint32_t>(), gb, gln, gt, ge, gm, cnt + 2, c->gspl.as<uint32_t>(), p.walk_bits,
                               p.split, p.refw ? 0 : 1);
  if (int r = mark(c, sd, "seg_walk")) return r;
  zs_k_seg_plan<<<ng, 64, 0, sd>>>(b.in, b.in_off, b.in_len, b.out_cap, gl, ng, wbits, p.refw ? 1 : 0, gb, gln, ge, gm,
                                   c->gpbase.as<uint32_t>(), c->gplist.as<uint4>());
  if (int r = mark(c, sd, "seg_plan")) return r;
  auto decode = p.d64 ? zs_k_seg_decode<true, false> : p.refw ? zs_k_seg_decode<false, true> : zs_k_seg_decode<false, false>;
  decode<<<p.gdec, 64, 0, sd>>>(b.in, b.in_off, b.in_len, gl, cnt + 2, spl, gb, gln, gt, gm, sb, scr);
  if (int r = mark(c, sd, "seg_decode")) return r;
  const int rsm = p.rsmall ? 65536 : 32768;
  auto resolve = p.rsmall ? zs_k_seg_resolve<512u, 65536u> : zs_k_seg_resolve<256u, 32768u>;
  HIPCHK(hipFuncSetAttribute((const void*)resolve, hipFuncAttributeMaxDynamicSharedMemorySize, rsm));
  resolve<<<ng, p.rsmall ? 512u : 256u, rsm, sd>>>(gl, gm, c->gpbase.as<uint32_t>(), c->gplist.as<uint4>(), sb, scr, b.out,
                                             b.out_off, lres, llen, cnt + 1, cnt + 3, c->gflist.as<uint32_t>());
  if (int r = mark(c, sd, "seg_resolve")) return r;
  // members the pieces could not finish: the wave kernel (skip_done), then the exact kernel
  const size_t wsm = zs_inflate_wave_lds_bytes(p.d64);
  auto wave = p.refw ? zs_k_inflate_wave<true> : zs_k_inflate_wave<false>;
  HIPCHK(hipFuncSetAttribute((const void*)wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wsm));
  wave<<<p.gfb, 64, wsm, sd>>>(b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, wbits, c->gflist.as<uint32_t>(),
                               ng, lres, llen, cnt + 3);
  HIPCHK(hipGetLastError());
  if (int r = mark(c, sd, "seg_fallback")) return r;
  return ZS_OK;
}

// The split decode of the members in c->ip.split (inflate_split.hip), on the third
// stream (high priority), beside the segmented decode.
static int split_launch(zs_ctx* c, hipStream_t st, int wbits, const Batch& b, zs_lane_res* lres) {
  const zs_inflate_plan& p = c->ip;
  const uint32_t ns = (uint32_t)p.split.size();
  HIPCHK(c->slist.ensure(4ull * ns));
  HIPCHK(c->sfound.ensure(8ull * ZS_SPLIT_MAX * ns));
  HIPCHK(c->spres.ensure(sizeof(zs_split_piece_res) * ZS_SPLIT_MAX * ns));
  HIPCHK(c->sscr.ensure(2ull * ZS_SPLIT_MAX * p.piece_cap * ns));
  HIPCHK(c->smem.ensure(sizeof(zs_split_member) * ns));
  HIPCHK(c->sval.ensure(4ull * p.val_stride * ns + 16));
  HIPCHK(hipMemcpyAsync(c->slist.p, p.split.data(), 4ull * ns, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(c->fork, st));
  HIPCHK(hipStreamWaitEvent(c->side2, c->fork, 0));
  if (int r = mark(c, c->side2, "start")) return r;
  const uint32_t* sl = c->slist.as<uint32_t>();
  uint64_t* sf = c->sfound.as<uint64_t>();
  zs_split_piece_res* sp = c->spres.as<zs_split_piece_res>();
  zs_k_split_find<<<ns * ZS_SPLIT_MAX, 256, 0, c->side2>>>(b.in, b.in_off, b.in_len, sl, wbits, sf);
  if (int r = mark(c, c->side2, "split_find")) return r;
  const size_t ssm = zs_split_lds_bytes(wbits == -16);
  HIPCHK(hipFuncSetAttribute((const void*)zs_k_split_decode, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ssm));
  zs_k_split_decode<<<ns * ZS_SPLIT_MAX, 64, ssm, c->side2>>>(b.in, b.in_off, b.in_len, sl, wbits, sf, sp,
                                                              c->sscr.as<uint16_t>(), p.piece_cap);
  if (int r = mark(c, c->side2, "split_decode")) return r;
  zs_split_member* sm = c->smem.as<zs_split_member>();
  uint32_t* sv = c->sval.as<uint32_t>();
  zs_k_split_chain<<<(ns + 63) / 64, 64, 0, c->side2>>>(b.in_len, b.out_cap, sl, ns, sp, sm);
  zs_k_split_place<<<ns * ZS_SPLIT_MAX, 256, 0, c->side2>>>(sp, sm, c->sscr.as<uint16_t>(), p.piece_cap, sv, p.val_stride);
  // the jump and write grids cover the largest member (grid-stride beyond)
  const uint32_t gx = (uint32_t)std::min<uint64_t>(1024, (p.val_stride + 1023) / 1024);
  for (int k = 0; k < 6; k++) zs_k_split_jump<<<dim3(gx, ns), 256, 0, c->side2>>>(sm, sv, p.val_stride);
  zs_k_split_write<<<dim3(gx, ns), 256, 0, c->side2>>>(sl, sm, sv, p.val_stride, b.out, b.out_off);
  zs_k_split_final<<<(ns + 63) / 64, 64, 0, c->side2>>>(sl, ns, sm, lres, c->llen.as<uint32_t>());
  HIPCHK(hipGetLastError());
  if (int r = mark(c, c->side2, "split_resolve")) return r;
  HIPCHK(hipEventRecord(c->join2, c->side2));
  return ZS_OK;
}

// The wave-per-member kernel over the members in c->ip.wave -- or, for large ones, the lane kernel's
// call-tracking instance -- on the side stream, beside the lane kernel.
static int wave_launch(zs_ctx* c, hipStream_t st, int wbits, const Batch& b, zs_lane_res* lres) {
  const zs_inflate_plan& p = c->ip;
  const uint32_t nw = (uint32_t)p.wave.size();
  uint32_t* const llen = c->llen.as<uint32_t>();
  HIPCHK(c->wlist.ensure(4ull * nw));
  HIPCHK(hipMemcpyAsync(c->wlist.p, p.wave.data(), 4ull * nw, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(c->fork, st));
  HIPCHK(hipStreamWaitEvent(c->side, c->fork, 0));
  const size_t wsm = zs_inflate_wave_lds_bytes(wbits == -16);
  auto wave = p.wave_refw ? zs_k_inflate_wave<true> : zs_k_inflate_wave<false>;
  HIPCHK(hipFuncSetAttribute((const void*)wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wsm));
  if (int r = mark(c, c->side, "start")) return r;
  if (p.wave_lanes) {
    const uint32_t B2 = p.wave_lane.block;
    const size_t lsm2 = B2 * zs_inflate_lane_lds_bytes(p.wave_lane.rt != 0);
    auto lk2 = lane_kernel(p.wave_lane.rt, true);
    HIPCHK(hipFuncSetAttribute((const void*)lk2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lsm2));
    lk2<<<(nw + B2 - 1) / B2, B2, lsm2, c->side>>>(b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, wbits, nw,
                                                   (zs_lane_tabs*)c->ltabs.p, lres, llen, ZS_INF_REF_WRAP, 0u,
                                                   c->wlist.as<uint32_t>(), zs_dict_args{});
  } else {
    wave<<<nw, 64, wsm, c->side>>>(b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, wbits, c->wlist.as<uint32_t>(),
                                   nw, lres, llen, nullptr);
  }
  HIPCHK(hipGetLastError());
  if (int r = mark(c, c->side, p.wave_lanes ? "inflate_large" : "inflate_wave")) return r;
  HIPCHK(hipEventRecord(c->join, c->side));
  return ZS_OK;
}

// The results of an inflate batch, an array of n entries each: device memory (the device entries, a
// host call's chunks) or the caller's host arrays (the host entries).  check may be null.
struct InflateOut {
  int32_t *status, *phase, *msg;
  uint32_t *out_len, *consumed, *check;
};

// The launch sequence of a planned inflate batch (c->ip by the options o; h: its host arrays, b: its device
// arrays; dd: its dictionaries; ck, ck_map: the trailer check's plan and its part map's place).
static int inflate_launch(zs_ctx* c, const zs_route_opts& o, hipStream_t st, int wbits, const Batch& h, const Batch& b,
                          const zs_dict_args& dd, const zs_checksum_plan* ck, size_t ck_map, const InflateOut& out) {
  const zs_inflate_plan& p = c->ip;
  const uint32_t n = b.n;
  const bool fastp = o.inflate_fast;
  const size_t smem = zs_inflate_smem_bytes(wbits);
  HIPCHK(hipFuncSetAttribute((const void*)zs_k_inflate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  zs_lane_res* const lres = fastp ? c->lres.as<zs_lane_res>() : nullptr;
  const int lflags = o.inflate_ref_wrap ? ZS_INF_REF_WRAP : 0;
  MARK("start");
  if (fastp) {
    zs_lane_tabs* const lt = (zs_lane_tabs*)c->ltabs.p;
    uint32_t* const llen = c->llen.as<uint32_t>();
    if (!p.split.empty())
      if (const int r = split_launch(c, st, wbits, b, lres)) return r;
    // the segmented decode after the split kernels are queued: its grids would
    // otherwise fill the chip ahead of the split decode's few long pieces (C5-ii:
    // the 2.19 MB fixture's split decode took 8.0 ms beside it, 2.5 ms alone)
    if (!p.seg.empty()) {
      if (const int r = seg_launch(c, o, st, wbits, h, b, lres)) return r;
      // (the join below waits for the side stream's last kernel)
      if (p.wave.empty()) HIPCHK(hipEventRecord(c->join, c->side));
    }
    if (!p.wave.empty())
      if (const int r = wave_launch(c, st, wbits, b, lres)) return r;
    const uint32_t B = p.lane.block;
    const size_t lsm = B * zs_inflate_lane_lds_bytes(p.lane.rt != 0);
    // (a batch with dictionaries: the dictionary instances, for every member of it)
    auto lk = p.dict ? lane_kernel_dict(p.lane.rt) : lane_kernel(p.lane.rt, false);
    HIPCHK(hipFuncSetAttribute((const void*)lk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lsm));
    lk<<<(n + B - 1) / B, B, lsm, st>>>(b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, wbits, n, lt, lres, llen,
                                        lflags, p.wave_min, nullptr, dd);
    MARK("inflate_lane");
    // Members the single-call instance bailed on whose cap allows more than one
    // inflate() call of the reference (more than 32 KiB of input, or output past
    // 64 KiB): re-run by the call-tracking instance, here, before the exact kernel
    if (o.inflate_ref_wrap && wbits != -16) {
      const size_t lsmr = 64 * zs_inflate_lane_lds_bytes(false);
      auto lkr = p.dict ? zs_k_inflate_lane<0, true, true> : zs_k_inflate_lane<0, true>;
      HIPCHK(hipFuncSetAttribute((const void*)lkr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lsmr));
      lkr<<<(n + 63) / 64, 64, lsmr, st>>>(b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, wbits, n, lt, lres,
                                           llen, ZS_INF_REF_WRAP, p.wave_min, nullptr, dd);
      MARK("inflate_long");
    }
    if (p.wave_min) {
      if (!p.seg.empty() || !p.wave.empty()) HIPCHK(hipStreamWaitEvent(st, c->join, 0));
      if (!p.split.empty()) HIPCHK(hipStreamWaitEvent(st, c->join2, 0));
      MARK("inflate_join");  // the caller's stream waiting for the side streams beyond the lane kernel
    }
    if (wbits > 0) {  // trailer checks over the decoded bytes: adler32 (zlib) / crc32 (gzip)
      uint32_t* chk = llen + n;
      ck_launch(c, st, *ck, ck_map, n, b.out, b.out_off, llen, chk, wbits == 31 ? 2 : 1);
      zs_k_inflate_lane_verify<<<(n + 255) / 256, 256, 0, st>>>(lres, chk, n);
      MARK("inflate_check");
    }
  }
  zs_k_inflate<<<n, 64, smem, st>>>(b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, wbits,
                                    c->istate.as<zs_inflate_result>(), lres, lflags, dd);
  MARK("inflate");
  // the lane count of the call: zeroed ahead of its first batch, then every batch's finish adds to it
  if (!c->call.lanes_zeroed) HIPCHK(hipMemsetAsync(c->lstat.p, 0, 4, st));
  c->call.lanes_zeroed = true;
  zs_k_inflate_finish<<<(n + 255) / 256, 256, 0, st>>>(c->istate.as<zs_inflate_result>(), lres, out.status, out.phase,
                                                       out.msg, out.out_len, out.consumed, (int)n,
                                                       c->lstat.as<uint32_t>());
  HIPCHK(hipMemcpyAsync(c->lane_count_host, c->lstat.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(c->lane_ev, st));
  if (out.check)
    zs_k_inflate_check<<<(n + 255) / 256, 256, 0, st>>>(b.in, b.in_off, out.status, out.consumed, wbits, out.check, (int)n);
  MARK("finish");
  HIPCHK(hipGetLastError());
  return ZS_OK;  // timing marks are collected when queried (no wait here)
}

// A validated, non-empty device batch (a public call's, a chunk of a host call, the segments of a restart
// call): plan, ensure, upload, launch.  out_cap[i] is the member's capacity as the caller set it
// (Z_BUF_ERROR past it, exactly); the decoders store whole dwords, so the member's region must reach
// out_off[i] + out_cap[i] rounded up to 4: the device entries' own buffers with capacities that are
// multiples of 4, or the host entries' staging.  opts: the options that decide routes and instances, when
// they are not the context's.
static int inflate_batch(zs_ctx* c, int wbits, const Batch& h, const InflateOut& out, hipStream_t st, const DictIn* dict,
                         const zs_route_opts* opts) {
  const zs_route_opts& o = opts ? *opts : c->o;
  const uint32_t n = h.n;
  // the members' dictionaries (dict: the _dict entries), the distinct ones found once
  zs_dict_set& ds = c->dset;
  ds.any = false;
  if (dict) zs_dict_distinct(n, dict->off, dict->len, ds);
  const bool hasdict = ds.any;
  const bool fastp = o.inflate_fast;
  if (fastp) zs_plan_inflate(o, wbits, n, h.in_len, h.out_cap, c->ip, hasdict ? dict->len : nullptr);
  const zs_meta_layout ml(n);
  // behind the batch's metadata: the members' dictionary offsets, lengths and ids, the distinct ones' too
  const size_t nu = hasdict ? ds.uoff.size() : 0;
  auto up256 = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t m_doff = ml.bytes, m_dlen = m_doff + up256(8ull * n), m_did = m_dlen + up256(4ull * n),
               m_uoff = m_did + up256(4ull * n), m_ulen = m_uoff + up256(8ull * nu),
               m_end = hasdict ? m_ulen + up256(4ull * nu) : ml.bytes;
  // ... and the trailer check's part map (its lengths are the decoders': the capacities bound them)
  const zs_checksum_plan* ck;
  size_t ck_bytes;
  if (const int rc = ck_prepare(c, fastp && wbits > 0, n, h.out_cap, &ck, &ck_bytes)) return rc;
  HIPCHK(c->istate.ensure(sizeof(zs_inflate_result) * (size_t)n));
  if (fastp) {
    HIPCHK(c->ltabs.ensure(zs_inflate_lane_scratch_bytes() * (size_t)n));
    HIPCHK(c->lres.ensure(sizeof(zs_lane_res) * (size_t)n));
    HIPCHK(c->llen.ensure(8ull * n));
  }
  if (hasdict) HIPCHK(c->dadler.ensure(4ull * nu));
  HIPCHK(c->lstat.ensure(16));
  if (!c->lane_count_host) {
    HIPCHK(hipHostMalloc((void**)&c->lane_count_host, 64, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&c->lane_ev, hipEventDisableTiming));
  }
  Batch b;
  if (int r = upload_batch(c, st, ml, m_end + ck_bytes, h, &b, [&](uint8_t* hm) {
        ck_fill(ck, hm + m_end);
        if (!hasdict) return;
        memcpy(hm + m_doff, dict->off, 8ull * n);
        memcpy(hm + m_dlen, dict->len, 4ull * n);
        memcpy(hm + m_did, ds.id.data(), 4ull * n);
        memcpy(hm + m_uoff, ds.uoff.data(), 8ull * nu);
        memcpy(hm + m_ulen, ds.ulen.data(), 4ull * nu);
      }))
    return r;
  zs_dict_args dd = {};
  if (hasdict) {
    const uint8_t* dm = c->meta.as<uint8_t>();
    dd = {dict->d_dict, (const uint64_t*)(dm + m_doff), (const uint32_t*)(dm + m_dlen), (const uint32_t*)(dm + m_did),
          c->dadler.as<uint32_t>()};
    // DICTID (zlib): the adler32 of each distinct dictionary, once
    if (wbits == 15) {
      zs_k_checksum<<<(uint32_t)nu, 64, 0, st>>>(dict->d_dict, (const uint64_t*)(dm + m_uoff),
                                                 (const uint32_t*)(dm + m_ulen), c->dadler.as<uint32_t>(), 1);
      HIPCHK(hipGetLastError());
    }
  }
  return inflate_launch(c, o, st, wbits, h, b, dd, ck, m_end, out);
}

// zs_inflate_validate's findings, as the entries report them
static int inflate_fail(zs_inflate_err e) { return fail(ZS_STREAM_ERROR, "%s", zs_inflate_err_text(e)); }
// The arrays of a call as validation reads them (the host entries stage their own regions)
static zs_inflate_call inflate_call(const Batch& h, bool caller_regions, const DictIn* dict) {
  zs_inflate_call a;
  a.n = h.n;
  a.out_off = caller_regions ? h.out_off : nullptr;
  a.out_cap = h.out_cap;
  a.caller_regions = caller_regions;
  a.dict = dict != nullptr;
  a.dict_arrays = dict && dict->off && dict->len;
  a.dict_buf = dict && dict->d_dict;
  a.dict_len = a.dict_arrays ? dict->len : nullptr;
  return a;
}

// ---- The entries that decode a stream's PIECES as the members of one batch and join them per stream: the
// segments between restart points, a gzip file's members (4.14), the blocks of a BGZF range (4.17).
// pieces_begin: where each piece lies, decodes and belongs (the caller uploads these with its own arrays), and
// room for the pieces' results and the staging route's regions.
struct PieceRun {
  std::vector<uint64_t> src, ooff, dst;
  InflateOut seg;  // the pieces' results: 5 arrays of M
};
static int pieces_begin(zs_ctx* c, const Batch& h, const zs_pieces& p, PieceRun& r) {
  const uint32_t M = p.M;
  r.src.resize(M);
  r.ooff.resize(M);
  r.dst.resize(M);
  for (uint32_t g = 0; g < M; g++) {
    const uint32_t i = p.rstream[g];
    r.src[g] = h.in_off[i] + p.soff[g];
    r.dst[g] = h.out_off[i] + p.opos[g];
    // (a piece without room stores nothing: it stays at its stream's start)
    r.ooff[g] = p.in_place ? h.out_off[i] + (p.ocap[g] ? p.opos[g] : 0u) : p.stoff[g];
  }
  HIPCHK(c->pres.ensure(20ull * M + 64));
  HIPCHK(c->pstage.ensure(p.stage_bytes));
  int32_t* const sr = c->pres.as<int32_t>();
  r.seg = {sr, sr + M, sr + 2 * M, (uint32_t*)(sr + 3 * M), (uint32_t*)(sr + 4 * M), nullptr};
  return ZS_OK;
}
// pieces_decode: the pieces as M members of one batch (in, in_off, in_len: host arrays as inflate_batch's),
// decoded with zlib semantics -- behind a reset or a member's trailer there is no call boundary of the
// reference's to reproduce, whatever the context's inflate_ref_wrap says -- and, with d_ptile, moved from
// staging to their places where the route is staged (d_*: the uploaded r.ooff, p.ocap, r.dst, p.ptile).
static int pieces_decode(zs_ctx* c, hipStream_t st, int wbits, const Batch& h, const zs_pieces& p, const PieceRun& r,
                         const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* d_ooff,
                         const uint32_t* d_ocap, const uint64_t* d_dst, const uint32_t* d_ptile) {
  const uint32_t M = p.M;
  if (!M) return ZS_OK;
  uint8_t* const stage = c->pstage.as<uint8_t>();
  zs_route_opts o2 = c->o;
  o2.inflate_ref_wrap = false;
  const Batch hs = {M, in, in_off, in_len, p.in_place ? h.out : stage, r.ooff.data(), p.ocap.data()};
  if (const int ri = inflate_batch(c, wbits, hs, r.seg, st, nullptr, &o2)) return ri;
  if (d_ptile && !p.in_place) {
    if (p.ptile[M])
      zs_k_restart_place<<<std::min(p.ptile[M], 32u * c->o.ncu), 256, 0, st>>>(stage, d_ooff, d_ocap, r.seg.out_len, d_dst,
                                                                               d_ptile, M, h.out);
    MARK("restart_place");
  }
  return ZS_OK;
}
// The check value over the joined output, the lengths the stitch wrote; the pieces' own values
// are verified by the decoders.  The part map goes to the front of the metadata block, which the pieces'
// batch is done with in stream order.
static int stream_check(zs_ctx* c, hipStream_t st, const Batch& h, const uint64_t* d_out_off, const uint32_t* cklen,
                        uint32_t* check) {
  const zs_checksum_plan* ck;
  size_t ck_bytes;
  if (const int rc = ck_prepare(c, true, h.n, h.out_cap, &ck, &ck_bytes)) return rc;
  if (ck_bytes) {
    HIPCHK(c->meta.ensure(ck_bytes));
    c->hck.assign(ck_bytes, 0);
    ck_fill(ck, c->hck.data());
    HIPCHK(hipMemcpyAsync(c->meta.p, c->hck.data(), ck_bytes, hipMemcpyHostToDevice, st));
  }
  ck_launch(c, st, *ck, 0, h.n, h.out, d_out_off, cklen, check, 2);
  return ZS_OK;
}

// ---- restart points (inflateSync, inflate.ts:1267-1337): a stream's segments decoded as the
// members of one raw batch and joined per stream.  A fault of the arguments is reported before the
// context is looked at (restart_refused: zs_restart_validate, then the null context).
struct RestartIn {
  const uint64_t* first;  // host, n + 1 entries: stream i's points are (in[k], out[k]), k in first[i] .. first[i + 1]
  const uint32_t* in;     // host
  const uint32_t* out;    // host
};
static int restart_refused(zs_ctx* c, int wbits, const Batch& h, bool device_entry, const RestartIn& rs) {
  zs_restart_call a;
  a.n = h.n;
  a.in_len = h.in_len;
  a.out_off = device_entry ? h.out_off : nullptr;
  a.out_cap = h.out_cap;
  a.caller_regions = device_entry;
  a.rfirst = rs.first;
  a.rin = rs.in;
  a.rout = rs.out;
  if (const zs_restart_err e = zs_restart_validate(wbits, a)) return fail(ZS_STREAM_ERROR, "%s", zs_restart_err_text(e));
  return c ? ZS_OK : fail(ZS_STREAM_ERROR, "null context");
}

// The device decode of a validated, non-empty batch with restart points (regions as inflate_batch's).
static int restart_batch(zs_ctx* c, int wbits, const Batch& h, const InflateOut& out, hipStream_t st,
                         const RestartIn& rs) {
  const uint32_t n = h.n;
  zs_restart_plan& p = c->rp;
  zs_plan_restart(n, h.in_len, h.out_cap, rs.first, rs.in, rs.out, p);
  const uint32_t M = p.M;
  const zs_checksum_plan* ck;
  size_t ck_bytes;
  if (const int rc = ck_prepare(c, wbits > 0, n, h.out_cap, &ck, &ck_bytes)) return rc;
  PieceRun r;
  if (const int rc = pieces_begin(c, h, p, r)) return rc;
  HIPCHK(c->rgather.ensure(p.gather_bytes));
  HIPCHK(c->rmark.ensure(4ull * M + 16));
  HIPCHK(c->rsum.ensure(8ull * n + 16));
  // the segment batch's metadata block is inflate_batch's own (it uploads it); this call's section lies
  // behind it: what the restart kernels read of the streams and of the segments, then the streams' checksum map
  std::vector<uint8_t>& hs = c->hsec;
  hs.clear();
  const size_t base = zs_meta_layout(M).bytes;
  auto put = [&](const void* q, size_t bytes) { return base + zs_section_put(hs, q, bytes); };
  const size_t s_in_off = put(h.in_off, 8ull * n), s_in_len = put(h.in_len, 4ull * n), s_out_off = put(h.out_off, 8ull * n),
               s_over = put(p.over.data(), 4ull * n), s_rfirst = put(p.rfirst.data(), 4ull * (n + 1)),
               s_src = put(r.src.data(), 8ull * M), s_soff = put(p.soff.data(), 4ull * M),
               s_slen = put(p.slen.data(), 4ull * M), s_goff = put(p.goff.data(), 8ull * M),
               s_glen = put(p.glen.data(), 4ull * M), s_ooff = put(r.ooff.data(), 8ull * M),
               s_ocap = put(p.ocap.data(), 4ull * M), s_olen = put(p.olen.data(), 4ull * M),
               s_opos = put(p.opos.data(), 4ull * M), s_dst = put(r.dst.data(), 8ull * M),
               s_gtile = put(p.gtile.data(), 4ull * (M + 1)), s_ptile = put(p.ptile.data(), 4ull * (M + 1)),
               s_ck = put(nullptr, ck_bytes);
  ck_fill(ck, hs.data() + (s_ck - s_in_off));
  HIPCHK(c->meta.ensure(s_in_off + hs.size()));  // (before inflate_batch's own ensure, which then keeps the block)
  HIPCHK(hipMemcpyAsync(c->meta.as<uint8_t>() + s_in_off, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
  const uint8_t* dm = c->meta.as<uint8_t>();
  auto u32 = [&](size_t at) { return (const uint32_t*)(dm + at); };
  auto u64 = [&](size_t at) { return (const uint64_t*)(dm + at); };
  uint8_t* gather = c->rgather.as<uint8_t>();
  uint32_t* mark_ = c->rmark.as<uint32_t>();
  MARK("start");
  if (p.gtile[M])  // (32 workgroups per CU: grid-stride beyond)
    zs_k_restart_gather<<<std::min(p.gtile[M], 32u * c->o.ncu), 256, 0, st>>>(h.in, u64(s_src), u32(s_slen), u32(s_glen),
                                                                              u64(s_goff), u32(s_gtile), M, gather, mark_);
  MARK("restart_gather");
  HIPCHK(hipGetLastError());
  if (const int ri = pieces_decode(c, st, -15, h, p, r, gather, p.goff.data(), p.glen.data(), u64(s_ooff), u32(s_ocap),
                                   u64(s_dst), u32(s_ptile)))
    return ri;
  const InflateOut& seg = r.seg;
  uint32_t* sum = c->rsum.as<uint32_t>();
  uint32_t* want = sum + n;
  zs_k_restart_stitch<<<n, 64, 0, st>>>(h.in, u64(s_in_off), u32(s_in_len), u32(s_over), u32(s_rfirst), u32(s_soff),
                                        u32(s_slen), u32(s_olen), u32(s_opos), mark_, seg.status, seg.msg, seg.out_len,
                                        seg.consumed, wbits, n, out.status, out.phase, out.msg, out.out_len, out.consumed, want);
  // the check value over the joined output, the lengths the stitch wrote, against the trailer's
  if (wbits > 0) ck_launch(c, st, *ck, s_ck, n, h.out, u64(s_out_off), out.out_len, sum, wbits == 31 ? 2 : 1);
  zs_k_restart_check<<<(n + 255) / 256, 256, 0, st>>>(sum, want, wbits, n, out.status, out.phase, out.msg, out.out_len,
                                                      out.consumed, out.check);
  MARK("restart_stitch");
  HIPCHK(hipGetLastError());
  return ZS_OK;
}

// ---- The search of the entries that find their pieces from the bytes: restart points (inflateSync /
// syncsearch, inflate.ts:1267-1337), a gzip file's members (zlib's gz_look, gzread.c),
// BGZF blocks sized from their headers where those can be trusted.  The kind selects the
// scan's rule, the sizing and tail kernels, the marks' names and the two refusals' texts.
enum FoundKind { FOUND_SYNC, FOUND_MEMBERS, FOUND_BGZF };
static const struct {
  const char *scan, *size, *many, *unsettled;
} kFound[3] = {
    {"sync_scan", "sync_size", "too many restart candidates (more than 67,108,863 with the streams in one call)",
     "the restart candidates' list did not settle"},
    {"members_scan", "members_size", "too many member candidates (more than 67,108,863 with the streams in one call)",
     "the member candidates' list did not settle"},
    {"members_scan", "bgzf_size", "too many member candidates (more than 67,108,863 with the streams in one call)",
     "the member candidates' list did not settle"},
};
struct Found {
  std::vector<uint32_t> cand, first;  // first: the streams' first points (FOUND_SYNC)
  std::vector<zs_sync_rec> rec;
  std::vector<uint8_t> rtrusted;  // per record (FOUND_BGZF)
  std::vector<uint64_t> cfirst;
  const uint64_t* d_off = nullptr;  // the streams' offsets and lengths on the device (c->fmeta)
  const uint32_t* d_len = nullptr;
};
template <bool EMIT>
static void cand_scan(FoundKind kind, uint32_t grid, hipStream_t st, const uint8_t* in, const uint64_t* d_off,
                      const uint32_t* d_len, const uint32_t* d_first, const uint32_t* d_tile, uint32_t n, uint64_t* tcount,
                      uint32_t* cand, uint64_t cap) {
  if (kind == FOUND_SYNC) zs_k_sync_scan<EMIT><<<grid, 256, 0, st>>>(in, d_off, d_len, d_first, d_tile, n, tcount, cand, cap);
  else zs_k_members_scan<EMIT><<<grid, 256, 0, st>>>(in, d_off, d_len, d_tile, n, tcount, cand, cap);
}
// The scan's two passes and the sizing launch over the streams of h, st waited for, then the candidates, the
// lanes' records and (FOUND_BGZF) their trusted bytes on the host.  The candidate list has the size the calls
// before needed; when this call has more, the emit pass and the sizing run once more over the grown list
// (and st is waited for a second time).  first (FOUND_SYNC): the streams' first points where the caller has
// the bytes (the host entries), else zs_k_sync_first computes them.  first_mark: the name of the mark in front
// of the scan ("start": the call's first; a caller that has run something on st before names what that mark ends).
static int cand_search(zs_ctx* c, FoundKind kind, int wbits, const Batch& h, hipStream_t st, const uint32_t* first, Found& f,
                       const char* first_mark = "start") {
  const uint32_t n = h.n;
  const bool sync = kind == FOUND_SYNC;
  std::vector<uint32_t> sh16(n), stile;
  uint64_t tin = 0;
  for (uint32_t i = 0; i < n; i++) {
    sh16[i] = (uint32_t)(((uintptr_t)h.in + h.in_off[i]) & 15u);
    tin += h.in_len[i];
  }
  zs_plan_sync_tiles(n, h.in_len, sh16.data(), stile);
  const uint32_t T = stile[n];
  std::vector<uint8_t>& hm = c->hsec;
  hm.clear();
  const size_t m_off = zs_section_put(hm, h.in_off, 8ull * n), m_len = zs_section_put(hm, h.in_len, 4ull * n),
               m_first = sync ? zs_section_put(hm, first, 4ull * n) : 0, m_tile = zs_section_put(hm, stile.data(), 4ull * (n + 1));
  HIPCHK(c->fmeta.ensure(hm.size()));
  HIPCHK(c->ftile.ensure(8ull * T + 16));
  HIPCHK(c->fcand.ensure(4ull * (tin / 2048 + 1024)));
  HIPCHK(hipMemcpyAsync(c->fmeta.p, hm.data(), hm.size(), hipMemcpyHostToDevice, st));
  uint8_t* dm = c->fmeta.as<uint8_t>();
  const uint64_t* d_off = (const uint64_t*)(dm + m_off);
  const uint32_t* d_len = (const uint32_t*)(dm + m_len);
  uint32_t* d_first = (uint32_t*)(dm + m_first);
  const uint32_t* d_tile = (const uint32_t*)(dm + m_tile);
  uint64_t* tcount = c->ftile.as<uint64_t>();
  const uint32_t grid = std::max(1u, std::min(T, 32u * c->o.ncu));
  MARK(first_mark);
  if (sync && !first) zs_k_sync_first<<<(n + 255) / 256, 256, 0, st>>>(h.in, d_off, d_len, wbits, n, d_first);
  cand_scan<false>(kind, grid, st, h.in, d_off, d_len, d_first, d_tile, n, tcount, nullptr, 0);
  zs_k_flush_tiles<<<1, ZS_FLUSH_TILE, 0, st>>>(tcount, T + 1);
  HIPCHK(hipGetLastError());
  std::vector<uint64_t> tpre(T + 1);
  for (int round = 0;; round++) {
    const uint64_t cap = c->fcand.cap / 4;
    HIPCHK(c->frec.ensure(sizeof(zs_sync_rec) * (n + cap)));
    if (kind == FOUND_BGZF) HIPCHK(c->ftrust.ensure(n + cap));
    uint32_t* d_cand = c->fcand.as<uint32_t>();
    zs_sync_rec* d_rec = c->frec.as<zs_sync_rec>();
    cand_scan<true>(kind, grid, st, h.in, d_off, d_len, d_first, d_tile, n, tcount, d_cand, cap);
    MARK(kFound[kind].scan);
    // (a lane per stream and per place of the list: the lanes past the candidates' count return at once)
    const uint64_t lanes = std::min<uint64_t>(n + cap, ZS_RESTART_SEG_MAX);
    const uint32_t per = kind == FOUND_BGZF ? ZS_BGZF_THREADS : ZS_SYNC_LANES, blocks = (uint32_t)((lanes + per - 1) / per);
    if (sync)
      zs_k_sync_size<<<blocks, per, 0, st>>>(h.in, d_off, d_len, d_first, d_tile, n, tcount, d_cand, cap, c->o.sync_pass, d_rec);
    else if (kind == FOUND_MEMBERS)
      zs_k_members_size<<<blocks, per, 0, st>>>(h.in, d_off, d_len, d_tile, n, tcount, d_cand, cap, c->o.sync_pass, d_rec);
    else
      zs_k_bgzf_size<<<blocks, per, 0, st>>>(h.in, d_off, d_len, d_tile, n, tcount, d_cand, cap, c->o.sync_pass, d_rec,
                                             c->ftrust.as<uint8_t>());
    MARK(kFound[kind].size);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(tpre.data(), tcount, 8ull * (T + 1), hipMemcpyDeviceToHost));
    if (!zs_sync_count_ok(n, tpre[T])) return fail(ZS_STREAM_ERROR, "%s", kFound[kind].many);
    if (tpre[T] <= cap) break;
    if (round) return fail(ZS_MEM_ERROR, "%s", kFound[kind].unsettled);
    HIPCHK(c->fcand.ensure(4ull * tpre[T]));
  }
  const uint64_t C = tpre[T];
  f.cand.resize(C);
  f.rec.resize(n + C);
  if (C) HIPCHK(hipMemcpy(f.cand.data(), c->fcand.p, 4ull * C, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(f.rec.data(), c->frec.p, sizeof(zs_sync_rec) * (n + C), hipMemcpyDeviceToHost));
  if (sync) {
    f.first.resize(n);
    HIPCHK(hipMemcpy(f.first.data(), d_first, 4ull * n, hipMemcpyDeviceToHost));
  }
  if (kind == FOUND_BGZF) {
    f.rtrusted.resize(n + C);
    HIPCHK(hipMemcpy(f.rtrusted.data(), c->ftrust.p, n + C, hipMemcpyDeviceToHost));
  }
  f.cfirst.resize(n + 1);
  for (uint32_t i = 0; i <= n; i++) f.cfirst[i] = tpre[stile[i]];
  f.d_off = d_off;
  f.d_len = d_len;
  return ZS_OK;
}
// A tail round: the starts a bound stopped (tstream, tstart) once more, a lane each, to their streams' ends
// (zs_k_sync_tail, zs_k_members_tail); st is waited for and the lanes' records come back.
static int cand_tail(zs_ctx* c, FoundKind kind, const Batch& h, hipStream_t st, const Found& f,
                     const std::vector<uint32_t>& tstream, const std::vector<uint32_t>& tstart, std::vector<zs_sync_rec>& tail) {
  const uint32_t m = (uint32_t)tstream.size(), blocks = (m + ZS_SYNC_LANES - 1) / ZS_SYNC_LANES;
  const size_t t_start = (4ull * m + 255) & ~size_t(255);
  HIPCHK(c->ftail.ensure(2 * t_start + sizeof(zs_sync_rec) * m));
  uint8_t* dt = c->ftail.as<uint8_t>();
  const uint32_t *d_stream = (const uint32_t*)dt, *d_start = (const uint32_t*)(dt + t_start);
  zs_sync_rec* d_rec = (zs_sync_rec*)(dt + 2 * t_start);
  HIPCHK(hipMemcpyAsync(dt, tstream.data(), 4ull * m, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dt + t_start, tstart.data(), 4ull * m, hipMemcpyHostToDevice, st));
  if (kind == FOUND_SYNC) zs_k_sync_tail<<<blocks, ZS_SYNC_LANES, 0, st>>>(h.in, f.d_off, f.d_len, d_stream, d_start, m, d_rec);
  else zs_k_members_tail<<<blocks, ZS_SYNC_LANES, 0, st>>>(h.in, f.d_off, f.d_len, d_stream, d_start, m, d_rec);
  MARK(kind == FOUND_SYNC ? "sync_size" : "members_size");
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  tail.resize(m);
  HIPCHK(hipMemcpy(tail.data(), d_rec, sizeof(zs_sync_rec) * m, hipMemcpyDeviceToHost));
  return ZS_OK;
}

// ---- restart points found from the bytes.  A fault of the arguments is reported before the
// context is looked at (zs_sync_validate, then the null context).
static int sync_refused(zs_ctx* c, int wbits, const Batch& h, bool device_entry) {
  if (const zs_sync_err e = zs_sync_validate(wbits, inflate_call(h, device_entry, nullptr)))
    return fail(ZS_STREAM_ERROR, "%s", zs_sync_err_text(e));
  return c ? ZS_OK : fail(ZS_STREAM_ERROR, "null context");
}

// The device decode of a validated, non-empty batch that finds its own points (regions as inflate_batch's;
// first: as cand_search's).  The points are planned here, from the candidates and the lanes' records; st is
// waited for once more where a chain ends at a lane its bound stopped (zs_k_sync_tail).
static int sync_batch(zs_ctx* c, int wbits, const Batch& h, const InflateOut& out, hipStream_t st, const uint32_t* first) {
  const uint32_t n = h.n;
  Found f;
  if (const int rs = cand_search(c, FOUND_SYNC, wbits, h, st, first, f)) return rs;
  zs_sync_plan& p = c->yp;
  zs_plan_sync(n, h.in_len, f.first.data(), f.cfirst.data(), f.cand.data(), f.rec.data(), p);
  if (!p.tstream.empty()) {
    // chains that end at a lane its bound stopped: the whole tail's reach, then the plan again
    std::vector<zs_sync_rec> tail;
    if (const int rt = cand_tail(c, FOUND_SYNC, h, st, f, p.tstream, p.tstart, tail)) return rt;
    for (size_t k = 0; k < tail.size(); k++) f.rec[p.trec[k]].reach = std::max(f.rec[p.trec[k]].reach, tail[k].reach);
    zs_plan_sync(n, h.in_len, f.first.data(), f.cfirst.data(), f.cand.data(), f.rec.data(), p);
  }
  {  // the plan's points pass the restart entries' validation by construction: nothing is launched otherwise
    zs_restart_call a;
    a.n = n;
    a.in_len = h.in_len;
    a.out_cap = h.out_cap;
    a.rfirst = p.rfirst.data();
    a.rin = p.rin.data();
    a.rout = p.rout.data();
    if (const zs_restart_err e = zs_restart_validate(wbits, a))
      return fail(ZS_MEM_ERROR, "the found restart points are refused: %s", zs_restart_err_text(e));
  }
  c->call.sync = true;
  return restart_batch(c, wbits, h, out, st, {p.rfirst.data(), p.rin.data(), p.rout.data()});
}

// ---- a gzip file's members found from the bytes.  A fault of the arguments is reported before
// the context is looked at (zs_members_validate, then the null context).
static int members_refused(zs_ctx* c, int wbits, const Batch& h, bool device_entry) {
  if (const zs_members_err e = zs_members_validate(wbits, inflate_call(h, device_entry, nullptr)))
    return fail(ZS_STREAM_ERROR, "%s", zs_members_err_text(e));
  return c ? ZS_OK : fail(ZS_STREAM_ERROR, "null context");
}

// The device decode of a validated, non-empty gzip batch whose streams hold any number of members
// (regions as inflate_batch's).  The members are planned here, from the candidates and the lanes' records
// (cand_search); st is waited for once more per tail round (zs_k_members_tail).  The members then decode as
// ONE gzip batch on the caller's input and are joined per stream.
// FOUND_BGZF: the _bgzf entries' mode.  It differs in three places: the sizing launch is
// zs_k_bgzf_size, which trusts the headers it can; the plan's members get their flags (zs_plan_bgzf_trusted);
// the stitch reports a flagged member's capacity outcome as its header's lie.
static int members_batch(zs_ctx* c, const Batch& h, const InflateOut& out, hipStream_t st, FoundKind kind) {
  const uint32_t n = h.n;
  const bool bgzf = kind == FOUND_BGZF;
  Found f;
  if (const int rs = cand_search(c, kind, 31, h, st, nullptr, f)) return rs;
  zs_members_plan& p = c->mp;
  for (;;) {
    zs_plan_members(n, h.in_len, h.out_cap, f.cfirst.data(), f.cand.data(), f.rec.data(), p);
    if (p.tstream.empty()) break;
    // true members that hold more than sync_pass false candidates: sized to the stream's end, then the plan again
    std::vector<zs_sync_rec> tail;
    if (const int rt = cand_tail(c, kind, h, st, f, p.tstream, p.tstart, tail)) return rt;
    for (size_t k = 0; k < tail.size(); k++) {
      if (tail[k].how == ZS_SYNC_PASSED) return fail(ZS_MEM_ERROR, "%s", "a member's tail lane did not settle");
      f.rec[p.trec[k]] = tail[k];
    }
  }
  c->call.members = true;
  const uint32_t M = p.M;
  std::vector<uint8_t> trusted;  // per planned member
  // (a tail round replaces records of untrusted starts only: a trusted one is never PASSED)
  if (bgzf)
    c->call.bgzf_trusted +=
        zs_plan_bgzf_trusted(p, h.out_cap, f.cfirst.data(), f.cand.data(), f.rec.data(), f.rtrusted.data(), trusted);
  PieceRun r;
  if (const int rc = pieces_begin(c, h, p, r)) return rc;
  std::vector<uint8_t>& hs = c->hsec;
  hs.clear();
  const size_t g_first = zs_section_put(hs, p.rfirst.data(), 4ull * (n + 1)), g_soff = zs_section_put(hs, p.soff.data(), 4ull * M),
               g_opos = zs_section_put(hs, p.opos.data(), 4ull * M), g_ocap = zs_section_put(hs, p.ocap.data(), 4ull * M),
               g_ooff = zs_section_put(hs, r.ooff.data(), 8ull * M), g_dst = zs_section_put(hs, r.dst.data(), 8ull * M),
               g_ptile = zs_section_put(hs, p.ptile.data(), 4ull * (M + 1)), g_out = zs_section_put(hs, h.out_off, 8ull * n),
               g_trust = bgzf ? zs_section_put(hs, trusted.data(), M) : 0;
  HIPCHK(c->pseg.ensure(hs.size()));
  HIPCHK(c->plen.ensure(4ull * n + 16));
  HIPCHK(hipMemcpyAsync(c->pseg.p, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
  const uint8_t* dg = c->pseg.as<uint8_t>();
  auto u32 = [&](size_t at) { return (const uint32_t*)(dg + at); };
  auto u64 = [&](size_t at) { return (const uint64_t*)(dg + at); };
  if (const int ri = pieces_decode(c, st, 31, h, p, r, h.in, r.src.data(), p.slen.data(), u64(g_ooff), u32(g_ocap), u64(g_dst),
                                   u32(g_ptile)))
    return ri;
  const InflateOut& seg = r.seg;
  uint32_t* cklen = c->plen.as<uint32_t>();
  zs_k_members_stitch<<<n, 64, 0, st>>>(u32(g_first), u32(g_soff), u32(g_opos), seg.status, seg.phase, seg.msg, seg.out_len,
                                        seg.consumed, n, out.status, out.phase, out.msg, out.out_len, out.consumed, cklen,
                                        bgzf ? dg + g_trust : nullptr);
  HIPCHK(hipGetLastError());
  if (out.check)
    if (const int rc = stream_check(c, st, h, u64(g_out), cklen, out.check)) return rc;
  MARK("members_stitch");
  HIPCHK(hipGetLastError());
  return ZS_OK;
}

// ---- BGZF ranges by virtual offset.  The refusals: the _bgzf entries' in their order, then the
// virtual offsets' (zs_bgzf_range_validate), then the null context.
static int bgzf_range_refused(zs_ctx* c, int wbits, const Batch& h, bool device_entry, const uint64_t* vb,
                              const uint64_t* ve) {
  if (const zs_members_err e = zs_members_validate(wbits, inflate_call(h, device_entry, nullptr)))
    return fail(ZS_STREAM_ERROR, "%s", zs_members_err_text(e));
  if (const zs_bgzf_range_err e = zs_bgzf_range_validate(h.n, h.in_len, vb, ve))
    return fail(ZS_STREAM_ERROR, "%s", zs_bgzf_range_err_text(e));
  return c ? ZS_OK : fail(ZS_STREAM_ERROR, "null context");
}

// The device decode of a validated, non-empty batch of ranges (regions as inflate_batch's; several streams may
// name the same input bytes, which are only read).  The scan and the sizing run over the ranges' SLICES as over
// streams of their own (cand_search, st waited for once); the plan follows the trusted headers
// (zs_plan_bgzf_range); the planned blocks decode whole, as ONE gzip batch on the caller's input, into staging;
// the stitch writes the streams' fields and the place kernel moves the delivered bytes behind it.
// A slice with ue > 0 reaches 65,536 bytes behind ce (zs_bgzf_range_slice), which holds two or three blocks behind
// the one that is needed and cuts the last of them short: a start no header can size, so its lane would decode it
// (5.7 ms for one range).  So the slices are first cut at the end of the block at ce, read from its header
// (zs_k_bgzf_range_end; st is waited for once more) -- where that header cannot be trusted the slice stays as it is
// and the plan fails the stream.  trimmed: the caller has done so (the host entries, from the caller's bytes).
static int bgzf_range_batch(zs_ctx* c, const Batch& h, const uint64_t* vb, const uint64_t* ve, const InflateOut& out,
                            hipStream_t st, bool trimmed = false) {
  const uint32_t n = h.n;
  std::vector<uint8_t>& hs = c->hsec;
  std::vector<uint64_t> sl_off(n);
  std::vector<uint32_t> sl_len(n), rce(n);
  bool any_end = false, cut = false;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t off;
    zs_bgzf_range_slice(h.in_len[i], vb[i], ve[i], off, sl_len[i]);
    sl_off[i] = h.in_off[i] + off;
    rce[i] = (uint32_t)((ve[i] >> 16) - (vb[i] >> 16));
    any_end = any_end || rce[i] < sl_len[i];
  }
  if (any_end && !trimmed) {
    hs.clear();
    zs_section_put(hs, sl_off.data(), 8ull * n);
    const size_t e_len = zs_section_put(hs, sl_len.data(), 4ull * n), e_rce = zs_section_put(hs, rce.data(), 4ull * n),
                 e_end = hs.size();
    HIPCHK(c->ftail.ensure(e_end + 4ull * n));
    uint8_t* de = c->ftail.as<uint8_t>();
    HIPCHK(hipMemcpyAsync(de, hs.data(), e_end, hipMemcpyHostToDevice, st));
    MARK("start");
    zs_k_bgzf_range_end<<<n / 256 + 1, 256, 0, st>>>(h.in, (const uint64_t*)de, (const uint32_t*)(de + e_len),
                                                     (const uint32_t*)(de + e_rce), n, (uint32_t*)(de + e_end));
    HIPCHK(hipGetLastError());
    MARK("bgzf_range_end");
    HIPCHK(hipStreamSynchronize(st));
    std::vector<uint32_t> end(n);
    HIPCHK(hipMemcpy(end.data(), de + e_end, 4ull * n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++)
      if (end[i] > rce[i] && end[i] <= sl_len[i]) sl_len[i] = end[i];
    cut = true;
  }
  Found f;
  const Batch hsl = {n, h.in, sl_off.data(), sl_len.data(), h.out, h.out_off, h.out_cap};
  // (behind the cut the search's first mark ends the host's wait for the ends: "bgzf_range_wait")
  if (const int rs = cand_search(c, FOUND_BGZF, 31, hsl, st, nullptr, f, cut ? "bgzf_range_wait" : "start")) return rs;
  zs_bgzf_range_plan& p = c->brp;
  zs_plan_bgzf_range(n, h.out_cap, vb, ve, f.cfirst.data(), f.cand.data(), f.rec.data(), f.rtrusted.data(), p);
  const uint32_t M = p.M;
  for (uint32_t g = 0; g < M; g++) c->call.bgzf_trusted += p.trusted[g];
  PieceRun r;  // (never in place: every block decodes whole at its region of staging, r.ooff = p.stoff)
  if (const int rc = pieces_begin(c, h, p, r)) return rc;
  hs.clear();
  const size_t g_first = zs_section_put(hs, p.rfirst.data(), 4ull * (n + 1)), g_soff = zs_section_put(hs, p.soff.data(), 4ull * M),
               g_opos = zs_section_put(hs, p.opos.data(), 4ull * M), g_ocap = zs_section_put(hs, p.ocap.data(), 4ull * M),
               g_skip = zs_section_put(hs, p.skip.data(), 4ull * M), g_take = zs_section_put(hs, p.take.data(), 4ull * M),
               g_rstream = zs_section_put(hs, p.rstream.data(), 4ull * M), g_stoff = zs_section_put(hs, p.stoff.data(), 8ull * M),
               g_dst = zs_section_put(hs, r.dst.data(), 8ull * M), g_ptile = zs_section_put(hs, p.ptile.data(), 4ull * (M + 1)),
               g_out = zs_section_put(hs, h.out_off, 8ull * n), g_verdict = zs_section_put(hs, p.verdict.data(), 4ull * n),
               g_vcons = zs_section_put(hs, p.vcons.data(), 4ull * n), g_trust = zs_section_put(hs, p.trusted.data(), M);
  HIPCHK(c->pseg.ensure(hs.size()));
  HIPCHK(c->plen.ensure(4ull * n + 16));
  HIPCHK(hipMemcpyAsync(c->pseg.p, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
  const uint8_t* dg = c->pseg.as<uint8_t>();
  auto u32 = [&](size_t at) { return (const uint32_t*)(dg + at); };
  auto u64 = [&](size_t at) { return (const uint64_t*)(dg + at); };
  // (the blocks as M gzip members; their delivered bytes are placed behind the stitch, by this entry's own kernel)
  if (const int ri = pieces_decode(c, st, 31, h, p, r, h.in, r.src.data(), p.slen.data(), nullptr, nullptr, nullptr, nullptr))
    return ri;
  const InflateOut& seg = r.seg;
  uint32_t* cklen = c->plen.as<uint32_t>();
  zs_k_bgzf_range_stitch<<<n, 64, 0, st>>>(u32(g_first), u32(g_soff), u32(g_opos), u32(g_take), u32(g_verdict), u32(g_vcons),
                                           seg.status, seg.phase, seg.msg, seg.consumed, n, out.status, out.phase, out.msg,
                                           out.out_len, out.consumed, cklen, dg + g_trust);
  HIPCHK(hipGetLastError());
  MARK("members_stitch");
  if (p.ptile[M])
    zs_k_bgzf_range_place<<<std::min(p.ptile[M], 32u * c->o.ncu), 256, 0, st>>>(
        c->pstage.as<uint8_t>(), u64(g_stoff), u32(g_ocap), seg.out_len, u32(g_skip), u32(g_take), u32(g_opos),
        u32(g_rstream), out.out_len, u64(g_dst), u32(g_ptile), M, h.out);
  HIPCHK(hipGetLastError());
  MARK("bgzf_range_place");
  if (out.check) {  // the check value over the delivered bytes
    if (const int rc = stream_check(c, st, h, u64(g_out), cklen, out.check)) return rc;
    HIPCHK(hipGetLastError());
    MARK("checksum");
  }
  return ZS_OK;
}

// The device entries' prologue, behind their refusals.  True: the call has begun and *st is its stream; else *rc
// is the entry's result (a HIP error, or ZS_OK for an empty batch).
static bool device_begin(zs_ctx* c, uint32_t n, void* hip_stream, hipStream_t* st, int* rc) {
  const hipError_t e = hipSetDevice(c->device);
  *rc = e == hipSuccess ? ZS_OK : fail(ZS_MEM_ERROR, "%s", hipGetErrorString(e));
  if (e != hipSuccess || n == 0) return false;
  call_begin(c, CALL_INFLATE);
  *st = hip_stream ? (hipStream_t)hip_stream : c->stream;
  return true;
}

// The shared body of the public device entries: the call begins once it is neither refused nor empty.
static int inflate_device(zs_ctx* c, int wbits, const Batch& h, const InflateOut& out, void* hip_stream,
                          const DictIn* dict, const RestartIn* rs) {
  if (!rs)  // (a restart call has passed restart_refused)
    if (const zs_inflate_err e = zs_inflate_validate(c != nullptr, wbits, inflate_call(h, true, dict))) return inflate_fail(e);
  hipStream_t st;
  int rc;
  if (!device_begin(c, h.n, hip_stream, &st, &rc)) return rc;
  return rs ? restart_batch(c, wbits, h, out, st, *rs) : inflate_batch(c, wbits, h, out, st, dict, nullptr);
}

// The host decode of every zs_inflate_batch* entry (h, out, dict: the caller's host memory): what the whole
// batch decides before anything is staged, the dictionaries to the device once, then the call begins and
// host_batch runs its chunks, each a device batch with a copy of the caller's exact capacities as the limits.
enum HostRoute { HOST_PLAIN, HOST_RESTART, HOST_SYNC, HOST_MEMBERS, HOST_BGZF };  // (HOST_RESTART: rs is given)
static int inflate_host(zs_ctx* c, int wbits, const Batch& h, const InflateOut& out, const DictIn* dict,
                        const RestartIn* rs, HostRoute route) {
  // (a restart call has passed restart_refused, one that finds its points sync_refused, its members members_refused)
  if (route == HOST_PLAIN)
    if (const zs_inflate_err e = zs_inflate_validate_host(c != nullptr, wbits, inflate_call(h, false, dict)))
      return inflate_fail(e);
  HIPCHK(hipSetDevice(c->device));
  const uint32_t n = h.n;
  if (n == 0) return ZS_OK;
  std::vector<uint64_t> poff;
  if (dict)
    if (const int r = host_dict_upload(c, n, *dict, poff)) return r;
  const std::vector<uint32_t> creq(h.out_cap, h.out_cap + n);
  call_begin(c, CALL_INFLATE);
  uint32_t* res[6] = {(uint32_t*)out.status, (uint32_t*)out.phase, (uint32_t*)out.msg, out.out_len, out.consumed, out.check};
  return host_batch(c, h, 6, res, 3,
                    [&](uint32_t a, uint32_t b, const uint64_t* doff, const uint64_t* ooff, uint32_t** dr) {
                      const Batch hb = {b - a, c->d_in.as<uint8_t>(), doff, h.in_len + a, c->d_out.as<uint8_t>(), ooff,
                                        creq.data() + a};
                      const InflateOut d = {(int32_t*)dr[0], (int32_t*)dr[1], (int32_t*)dr[2], dr[3], dr[4],
                                            out.check ? dr[5] : nullptr};
                      // (a chunk's points and dictionaries: the same arrays, the chunk's part of the index)
                      if (route == HOST_RESTART) return restart_batch(c, wbits, hb, d, c->stream, {rs->first + a, rs->in, rs->out});
                      if (route == HOST_MEMBERS) return members_batch(c, hb, d, c->stream, FOUND_MEMBERS);
                      if (route == HOST_BGZF) return members_batch(c, hb, d, c->stream, FOUND_BGZF);
                      if (route == HOST_SYNC) {  // the first points where the bytes are: the caller's memory
                        std::vector<uint32_t> first(b - a);
                        for (uint32_t i = a; i < b; i++)
                          first[i - a] = std::min(zs_wrapper_header_len(wbits, h.in + h.in_off[i], h.in_len[i]), h.in_len[i]);
                        return sync_batch(c, wbits, hb, d, c->stream, first.data());
                      }
                      const DictIn di = dict ? DictIn{c->d_dict.as<uint8_t>(), poff.data() + a, dict->len + a} : DictIn{};
                      return inflate_batch(c, wbits, hb, d, c->stream, dict ? &di : nullptr, nullptr);
                    },
                    route >= HOST_SYNC);
}

extern "C" int zs_inflate_batch_device_ex(zs_ctx* c, int wbits, uint32_t n, const uint8_t* d_in,
                                          const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                          const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                          int32_t* d_phase, int32_t* d_msg, uint32_t* d_out_len,
                                          uint32_t* d_consumed, uint32_t* d_check, void* hip_stream) {
  return inflate_device(c, wbits, {n, d_in, in_off, in_len, d_out, out_off, out_cap},
                        {d_status, d_phase, d_msg, d_out_len, d_consumed, d_check}, hip_stream, nullptr, nullptr);
}

extern "C" int zs_inflate_batch_device(zs_ctx* c, int wbits, uint32_t n, const uint8_t* d_in, const uint64_t* in_off,
                                       const uint32_t* in_len, uint8_t* d_out, const uint64_t* out_off,
                                       const uint32_t* out_cap, int32_t* d_status, int32_t* d_phase, int32_t* d_msg,
                                       uint32_t* d_out_len, uint32_t* d_consumed, void* hip_stream) {
  return zs_inflate_batch_device_ex(c, wbits, n, d_in, in_off, in_len, d_out, out_off, out_cap, d_status, d_phase,
                                    d_msg, d_out_len, d_consumed, nullptr, hip_stream);
}

extern "C" int zs_inflate_batch(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                const uint32_t* in_len, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                int32_t* status, int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed) {
  return zs_inflate_batch_ex(c, wbits, n, in, in_off, in_len, out, out_off, out_cap, status, phase, msg, out_len,
                             consumed, nullptr);
}

extern "C" int zs_inflate_batch_ex(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                   const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                   const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                   uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  return inflate_host(c, wbits, {n, in, in_off, in_len, out, out_off, out_cap},
                      {status, phase, msg, out_len, consumed, check}, nullptr, nullptr, HOST_PLAIN);
}

// inflate.ts:1267-1337 -- device buffers
extern "C" int zs_inflate_batch_restart_device(zs_ctx* c, int wbits, uint32_t n, const uint8_t* d_in,
                                               const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                               const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                               int32_t* d_phase, int32_t* d_msg, uint32_t* d_out_len,
                                               uint32_t* d_consumed, uint32_t* d_check, void* hip_stream,
                                               const uint64_t* restart_first, const uint32_t* restart_in,
                                               const uint32_t* restart_out) {
  const Batch h = {n, d_in, in_off, in_len, d_out, out_off, out_cap};
  const RestartIn rs = {restart_first, restart_in, restart_out};
  if (const int r = restart_refused(c, wbits, h, true, rs)) return r;
  return inflate_device(c, wbits, h, {d_status, d_phase, d_msg, d_out_len, d_consumed, d_check}, hip_stream, nullptr, &rs);
}

// inflate.ts:1267-1337 -- host buffers
extern "C" int zs_inflate_batch_restart(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                        const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                        const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                        uint32_t* out_len, uint32_t* consumed, uint32_t* check,
                                        const uint64_t* restart_first, const uint32_t* restart_in,
                                        const uint32_t* restart_out) {
  const Batch h = {n, in, in_off, in_len, out, out_off, out_cap};
  const RestartIn rs = {restart_first, restart_in, restart_out};
  if (const int r = restart_refused(c, wbits, h, false, rs)) return r;
  return inflate_host(c, wbits, h, {status, phase, msg, out_len, consumed, check}, nullptr, &rs, HOST_RESTART);
}

// inflate.ts:1267-1337 -- the points found from the bytes; device buffers
extern "C" int zs_inflate_batch_sync_device(zs_ctx* c, int wbits, uint32_t n, const uint8_t* d_in, const uint64_t* in_off,
                                            const uint32_t* in_len, uint8_t* d_out, const uint64_t* out_off,
                                            const uint32_t* out_cap, int32_t* d_status, int32_t* d_phase,
                                            int32_t* d_msg, uint32_t* d_out_len, uint32_t* d_consumed,
                                            uint32_t* d_check, void* hip_stream) {
  const Batch h = {n, d_in, in_off, in_len, d_out, out_off, out_cap};
  if (const int r = sync_refused(c, wbits, h, true)) return r;
  hipStream_t st;
  int rc;
  if (!device_begin(c, n, hip_stream, &st, &rc)) return rc;
  return sync_batch(c, wbits, h, {d_status, d_phase, d_msg, d_out_len, d_consumed, d_check}, st, nullptr);
}

// ... host buffers
extern "C" int zs_inflate_batch_sync(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                     const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                     const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                     uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  const Batch h = {n, in, in_off, in_len, out, out_off, out_cap};
  if (const int r = sync_refused(c, wbits, h, false)) return r;
  return inflate_host(c, wbits, h, {status, phase, msg, out_len, consumed, check}, nullptr, nullptr, HOST_SYNC);
}

// The points the last call on the context found, in the layout the restart entries take: restart_first
// (n + 1 entries, from 0), then at most `cap` points.  0 when the last inflate call found none itself.
extern "C" uint64_t zs_last_restart_points(zs_ctx* c, uint64_t* restart_first, uint32_t* restart_in,
                                           uint32_t* restart_out, uint64_t cap) {
  if (!c || !c->call.sync) return 0;
  const zs_sync_plan& p = c->yp;
  if (restart_first) memcpy(restart_first, p.rfirst.data(), 8ull * p.rfirst.size());
  const uint64_t k = std::min<uint64_t>(cap, p.rin.size());
  if (restart_in) memcpy(restart_in, p.rin.data(), 4ull * k);
  if (restart_out) memcpy(restart_out, p.rout.data(), 4ull * k);
  return p.rin.size();
}

// zlib's gz_look (gzread.c): every member of a gzip file; device buffers
extern "C" int zs_inflate_batch_members_device(zs_ctx* c, int wbits, uint32_t n, const uint8_t* d_in,
                                               const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                               const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                               int32_t* d_phase, int32_t* d_msg, uint32_t* d_out_len,
                                               uint32_t* d_consumed, uint32_t* d_check, void* hip_stream) {
  const Batch h = {n, d_in, in_off, in_len, d_out, out_off, out_cap};
  if (const int r = members_refused(c, wbits, h, true)) return r;
  hipStream_t st;
  int rc;
  if (!device_begin(c, n, hip_stream, &st, &rc)) return rc;
  return members_batch(c, h, {d_status, d_phase, d_msg, d_out_len, d_consumed, d_check}, st, FOUND_MEMBERS);
}

// ... host buffers
extern "C" int zs_inflate_batch_members(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                        const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                        const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                        uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  const Batch h = {n, in, in_off, in_len, out, out_off, out_cap};
  if (const int r = members_refused(c, wbits, h, false)) return r;
  return inflate_host(c, wbits, h, {status, phase, msg, out_len, consumed, check}, nullptr, nullptr, HOST_MEMBERS);
}

// BGZF files, the members sized from their headers where those can be trusted; device buffers
extern "C" int zs_inflate_batch_bgzf_device(zs_ctx* c, int wbits, uint32_t n, const uint8_t* d_in, const uint64_t* in_off,
                                            const uint32_t* in_len, uint8_t* d_out, const uint64_t* out_off,
                                            const uint32_t* out_cap, int32_t* d_status, int32_t* d_phase,
                                            int32_t* d_msg, uint32_t* d_out_len, uint32_t* d_consumed,
                                            uint32_t* d_check, void* hip_stream) {
  const Batch h = {n, d_in, in_off, in_len, d_out, out_off, out_cap};
  if (const int r = members_refused(c, wbits, h, true)) return r;
  hipStream_t st;
  int rc;
  if (!device_begin(c, n, hip_stream, &st, &rc)) return rc;
  return members_batch(c, h, {d_status, d_phase, d_msg, d_out_len, d_consumed, d_check}, st, FOUND_BGZF);
}

// ... host buffers
extern "C" int zs_inflate_batch_bgzf(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                     const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                     const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                     uint32_t* out_len, uint32_t* consumed, uint32_t* check) {
  const Batch h = {n, in, in_off, in_len, out, out_off, out_cap};
  if (const int r = members_refused(c, wbits, h, false)) return r;
  return inflate_host(c, wbits, h, {status, phase, msg, out_len, consumed, check}, nullptr, nullptr, HOST_BGZF);
}

// The planned members of the last _bgzf call on the context whose size came from their header; 0 after any
// other inflate call.  Known when the call returns: the plan is made on the host.
extern "C" uint64_t zs_last_bgzf_trusted(zs_ctx* c) { return c ? c->call.bgzf_trusted : 0; }

// Host arithmetic, no context: the trusted headers followed from 0 (zs_bgzf.h)
extern "C" int zs_bgzf_out_len(const uint8_t* in, uint32_t in_len, uint64_t* total) {
  uint64_t t = 0;
  const int r = in ? zs_bgzf_chain(in, in_len, t) : 0;
  if (total) *total = r ? t : 0;
  return r;
}

// BGZF ranges by virtual offset; device buffers.  hip_stream is waited for as in the _bgzf entry.
extern "C" int zs_inflate_batch_bgzf_range_device(zs_ctx* c, int wbits, uint32_t n, const uint8_t* d_in,
                                                  const uint64_t* in_off, const uint32_t* in_len,
                                                  const uint64_t* voff_begin, const uint64_t* voff_end, uint8_t* d_out,
                                                  const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                                  int32_t* d_phase, int32_t* d_msg, uint32_t* d_out_len,
                                                  uint32_t* d_consumed, uint32_t* d_check, void* hip_stream) {
  const Batch h = {n, d_in, in_off, in_len, d_out, out_off, out_cap};
  if (const int r = bgzf_range_refused(c, wbits, h, true, voff_begin, voff_end)) return r;
  hipStream_t st;
  int rc;
  if (!device_begin(c, n, hip_stream, &st, &rc)) return rc;
  return bgzf_range_batch(c, h, voff_begin, voff_end, {d_status, d_phase, d_msg, d_out_len, d_consumed, d_check}, st);
}

// ... host buffers: only each range's slice of its stream is staged, as a stream of its own whose range begins
// in its first block; the slices' results are the streams' but for consumed, which counts from the slice
extern "C" int zs_inflate_batch_bgzf_range(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                           const uint32_t* in_len, const uint64_t* voff_begin, const uint64_t* voff_end,
                                           uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                           int32_t* status, int32_t* phase, int32_t* msg, uint32_t* out_len,
                                           uint32_t* consumed, uint32_t* check) {
  const Batch h = {n, in, in_off, in_len, out, out_off, out_cap};
  if (const int r = bgzf_range_refused(c, wbits, h, false, voff_begin, voff_end)) return r;
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return ZS_OK;
  std::vector<uint64_t> sl_off(n), svb(n), sve(n);
  std::vector<uint32_t> sl_len(n), cb(n);
  for (uint32_t i = 0; i < n; i++) {
    zs_bgzf_range_slice(in_len[i], voff_begin[i], voff_end[i], cb[i], sl_len[i]);
    sl_off[i] = in_off[i] + cb[i];
    svb[i] = voff_begin[i] & 0xffffu;
    sve[i] = voff_end[i] - ((uint64_t)cb[i] << 16);
    // (the slice cut at the end of the block at ce, as bgzf_range_batch cuts it: read here, where the bytes are)
    const uint32_t rce = (uint32_t)(sve[i] >> 16);
    uint32_t e = 0, isize = 0;
    if (rce < sl_len[i] && zs_bgzf_header(in + sl_off[i], sl_len[i], rce, e, isize)) sl_len[i] = e;
  }
  const Batch hsl = {n, in, sl_off.data(), sl_len.data(), out, out_off, out_cap};
  const std::vector<uint32_t> creq(out_cap, out_cap + n);
  call_begin(c, CALL_INFLATE);
  uint32_t* res[6] = {(uint32_t*)status, (uint32_t*)phase, (uint32_t*)msg, out_len, consumed, check};
  const int rc = host_batch(c, hsl, 6, res, 3,
                            [&](uint32_t a, uint32_t b, const uint64_t* doff, const uint64_t* ooff, uint32_t** dr) {
                              const Batch hb = {b - a, c->d_in.as<uint8_t>(), doff, sl_len.data() + a,
                                                c->d_out.as<uint8_t>(), ooff, creq.data() + a};
                              const InflateOut d = {(int32_t*)dr[0], (int32_t*)dr[1], (int32_t*)dr[2], dr[3], dr[4],
                                                    check ? dr[5] : nullptr};
                              return bgzf_range_batch(c, hb, svb.data() + a, sve.data() + a, d, c->stream, true);
                            },
                            true);
  if (rc == ZS_OK && consumed)
    for (uint32_t i = 0; i < n; i++) consumed[i] += cb[i];
  return rc;
}

// Host arithmetic, no context: the rule of zs_plan_bgzf_range over the headers (zs_bgzf.h)
extern "C" int zs_bgzf_range_out_len(const uint8_t* in, uint32_t in_len, uint64_t voff_begin, uint64_t voff_end,
                                     uint64_t* total) {
  uint64_t t = 0;
  const int r = (in || !in_len) ? zs_bgzf_range_chain(in, in_len, voff_begin, voff_end, t) : 0;
  if (total) *total = r ? t : 0;
  return r;
}

// ... an uncompressed position's virtual offset from one stream's index of blocks
extern "C" int zs_bgzf_voffset(const uint32_t* block_in, const uint32_t* block_out, uint64_t count, uint64_t upos,
                               uint64_t* voff) {
  uint64_t v = 0;
  const int r = zs_bgzf_voffset_of(block_in, block_out, count, upos, v);
  if (voff) *voff = v;
  return r;
}

// The members the last _members or _bgzf call on the context decoded, in the layout of zs_last_restart_points:
// member_first (n + 1 entries, from 0), then at most `cap` members' (in_pos, out_pos), every stream's
// member 0 = (0, 0) included.  0 when the last inflate call on the context was no _members call.
extern "C" uint64_t zs_last_members(zs_ctx* c, uint64_t* member_first, uint32_t* member_in, uint32_t* member_out,
                                    uint64_t cap) {
  if (!c || !c->call.members) return 0;
  const zs_members_plan& p = c->mp;
  if (member_first)
    for (size_t i = 0; i < p.rfirst.size(); i++) member_first[i] = p.rfirst[i];
  const uint64_t k = std::min<uint64_t>(cap, p.M);
  if (member_in) memcpy(member_in, p.soff.data(), 4ull * k);
  if (member_out) memcpy(member_out, p.opos.data(), 4ull * k);
  return p.M;
}

extern "C" uint32_t zs_wrapper_header_len(int wbits, const uint8_t* in, uint32_t in_len) {
  return zs_wrapper_header_len_of(wbits, in, in_len);
}

// The index of the last flushed compress call on the context: for every flush point, in the order of
// flush_pos, the offset in its stream's output of the byte behind the marker -- the wrapper's header,
// then the bytes of the segments before it (zs_k_flush_local's scan, which zs_k_flush_place rebases
// the blocks by).  A host entry's chunks follow each other.
extern "C" uint64_t zs_last_flush_index(zs_ctx* c, uint32_t* in_pos, uint64_t cap) {
  if (!c || c->call.fidx.empty() || c->call.fidx[0].bgzf || !c->fscan.p) return 0;
  if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 0;
  std::vector<uint64_t> scan(c->call.fscan_used);
  if (hipMemcpy(scan.data(), c->fscan.p, 8ull * scan.size(), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  uint64_t k = 0;
  for (const zs_ctx::FlushIdx& f : c->call.fidx) {
    const uint64_t* segx = scan.data() + f.at;
    const uint64_t* tile = segx + f.M + 1;
    auto at = [&](uint32_t x) { return tile[x / ZS_FLUSH_TILE] + segx[x]; };  // the bytes of all segments before x
    for (uint32_t s = 0; s < f.n; s++)
      for (uint32_t g = f.sfirst[s] + 1; g < f.sfirst[s + 1]; g++, k++)
        if (in_pos && k < cap) in_pos[k] = (uint32_t)(f.hl + (at(g) - at(f.sfirst[s])));
  }
  return k;
}

// ---- preset dictionaries (inflateSetDictionary, inflate.ts:1220-1249; Z_NEED_DICT, inflate.ts:594-597)
extern "C" int zs_inflate_batch_dict_device(zs_ctx* c, int wbits, uint32_t n, const uint8_t* d_in,
                                            const uint64_t* in_off, const uint32_t* in_len, uint8_t* d_out,
                                            const uint64_t* out_off, const uint32_t* out_cap, int32_t* d_status,
                                            int32_t* d_phase, int32_t* d_msg, uint32_t* d_out_len,
                                            uint32_t* d_consumed, uint32_t* d_check, void* hip_stream,
                                            const uint8_t* d_dict, const uint64_t* dict_off,
                                            const uint32_t* dict_len) {
  const DictIn di = {d_dict, dict_off, dict_len};
  return inflate_device(c, wbits, {n, d_in, in_off, in_len, d_out, out_off, out_cap},
                        {d_status, d_phase, d_msg, d_out_len, d_consumed, d_check}, hip_stream, &di, nullptr);
}

extern "C" int zs_inflate_batch_dict(zs_ctx* c, int wbits, uint32_t n, const uint8_t* in, const uint64_t* in_off,
                                     const uint32_t* in_len, uint8_t* out, const uint64_t* out_off,
                                     const uint32_t* out_cap, int32_t* status, int32_t* phase, int32_t* msg,
                                     uint32_t* out_len, uint32_t* consumed, uint32_t* check, const uint8_t* dict,
                                     const uint64_t* dict_off, const uint32_t* dict_len) {
  const DictIn di = {dict, dict_off, dict_len};  // (host memory here)
  return inflate_host(c, wbits, {n, in, in_off, in_len, out, out_off, out_cap},
                      {status, phase, msg, out_len, consumed, check}, &di, nullptr, HOST_PLAIN);
}
