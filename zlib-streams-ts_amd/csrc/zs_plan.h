// zs_plan.h -- what the host layer (capi.cpp) decides about a batch before it
// launches anything: each member's route, the kernel instances, the grids and
// the workspace sizes.  Pure functions of the options and the batch's lengths:
// no HIP types, no HIP calls, so the host check compiles them with a plain C++
// compiler (tools/emu/emu_plan.cpp, tests/test_plan_model.py).  capi.cpp runs
// plan, then the ensure calls, then the uploads and launches.
#ifndef ZS_PLAN_H
#define ZS_PLAN_H
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "zs_common.h"
#include "zs_sweep_ring.h"  // zs_sweep_uniform8

#if defined(__HIPCC__)
#define ZS_PLAN_FN static __host__ __device__ inline
#else
#define ZS_PLAN_FN static inline
#endif

// ---- constants shared with the kernels
#define ZS_SPLIT_MAX 64u           // bit ranges searched per member (pieces <= this)
#define ZS_SEG_LANES 64u    // pieces per span (one lane each)
#define ZS_SEG_W 1024u      // bits of a lane's start window whose symbol starts it records (the sync bitmaps; 2048 in
                            // the walk instance for batches of few large members: fewer chains that do not meet)
#define ZS_SEG_PAD 16u      // u16 values of padding behind each piece's scratch
#define ZS_SEG_BIG_BITS (1u << 21)  // members with more input bits: block starts from the finder as extra entries
#define ZS_SEG_SPLIT_BITS (1u << 18)  // deflate64 members with more input bits: the split decode (long copies)
#define ZS_SEG_BLOCK_BITS 16384u    // span slots per member: one per this many input bits (+ zs_seg_spans' margin)
#define ZS_SEG_SMAX 8192u           // bits per lane at most (a span's lanes: seg_bits, then from the block before)
// levels 4..9 (deflate_sweep.hip), one workgroup per WINDOW: the inserted
// positions from `base` up to its own positions' end ohi (at most 65,535; a
// stream of up to 65,537 bytes is one window, base 0); the window writes the
// results of its own positions [olo, ohi) (window-relative), members at
// members + mb (u16, window-relative)
struct zs_sweep_seg {
  uint32_t s, base, olo, ohi;
  uint64_t mb;
  uint64_t pad;
};
#define ZS_SEG_WPOS 65535u   // inserted positions per window at most (u16 members; bucket counts fit 16 bits)
#define ZS_SEG_FIRST 65520u  // own positions of a long stream's first window ...
#define ZS_SEG_OWN 32752u    // ... and of its later ones, after a 32,768-position look-back (> MAX_DIST);
                             // multiples of 16: every window starts 16-byte aligned with its stream
// parse scratch words per 1024-position segment (deflate_parse.hip)
#define ZS_PARSE_SEG 1024u
#define ZS_PARSE_SEG_WORDS 3596u
#define ZS_PARSE2W_SEG 512u
#define ZS_PARSE2W_SEG_WORDS 2060u
#define ZS_PARSE4W_SEG 256u
#define ZS_PARSE4W_SEG_WORDS 1292u
#define ZS_PARSE2W_AUTO 2048u  // batches below this many streams parse with two waves per stream (option parse_waves = 0)

// A member the lane kernel leaves to the large-member paths (the segmented, split
// or wave decode) when wave_min is set: more input bytes than wave_min, or a high
// expansion (a cap past 64 KiB and at least 8 bytes of it per input byte: long
// copies, which one lane makes byte by byte -- deflate64's zeros_100k.deflate64 took a
// lane 4.3 ms; the wave decoders copy 64 bytes at a time)
ZS_PLAN_FN bool zs_inf_expands(uint32_t in_len, uint32_t out_cap) {
  return out_cap > 65536u && out_cap / 8u >= in_len;
}
ZS_PLAN_FN bool zs_inf_large(uint32_t in_len, uint32_t out_cap, uint32_t wave_min) {
  return wave_min && (in_len > wave_min || zs_inf_expands(in_len, out_cap));
}

// ---- the options that decide routes and instances (zs_set_option)
struct zs_route_opts {
  bool inflate_fast = true;
  bool inflate_ref_wrap = true;  // reproduce the reference's inflate_fast window-wrap copy (inffast.ts:133-147)
  // split decode of large members (inflate_split.hip): deflate64, or raw deflate without the window-wrap copy
  bool inflate_split = true;
  // segmented decode (inflate_seg.hip): a member's blocks cut into lane-sized pieces that synchronise
  bool inflate_seg = true;
  uint32_t inflate_wave_min = 32768;  // members with more input bytes decode one per wave (inflate_wave.hip); 0: never
  uint32_t lane_large_min = 2304;     // this many large members or more: one LANE each (zs_k_inflate_lane<.., true>); 256 KiB members: wave kernel 26.9 / 68.5 / 128 ms at 1024 / 2048 / 4096, lanes 68.6 / 78.3 / 77.7
  int lane_block = 0;        // members per workgroup of the inflate lane path (0: chosen from the batch size)
  uint32_t seg_bits = 0;            // input bits per lane of an entry's first block (later ones: from the block before);
                                    // 0: 4096 for members of 64 KiB of input or more on average, else 2048
  uint32_t seg_small_batch = 16384; // batches of at most this many members ...
  uint32_t seg_small_min = 4096;    // ... send members with more input bytes than this to it too
  bool seg_wide = true;             // the 2048-bit sync window for a batch of few large members
  int seg_split = 2;                // pieces cut in two at the walk's mid points (0 off, 1 on, 2 auto: small batches)
  uint32_t seg_big_bits = ZS_SEG_BIG_BITS;  // members with more input bits also walk from the finder's block starts
  uint64_t seg_scratch_max = 16ull << 30;  // bytes of u16 piece scratch the segmented decode may take per batch
  uint32_t ncu = 256;               // compute units of the device
  int parse_waves = 0;       // L4..9 one-wave parse: waves per stream (1, 2; 0: chosen from the batch size)
  bool match_sweep = true;   // 0: the chain-walk kernels for every stream (a cross-check of the sweep)
  // Z_RLE: 1 reproduces the reference's deflate_rle, whose scan compares the previous byte's value
  // with the scan index (deflate.ts:1469-1481) and so finds no run: deflate_huff's tally; 0: zlib's
  bool rle_ref = true;
  // the data checksums (zs_plan_checksum): a batch with a stream longer than checksum_split bytes
  // runs in parts of checksum_part bytes (0: never; measured)
  uint32_t checksum_split = 1u << 18;
  uint32_t checksum_part = 65536;  // a power of two, ZS_CK_PART_MIN .. ZS_CK_PART_MAX
  // the host-buffer entries' pipeline (zs_plan_host_chunks, zs_plan_host_pack0)
  uint64_t host_chunk_min = 32ull << 20;  // input bytes from which a batch of ZS_HOST_CHUNK_STREAMS runs as four chunks; 0: never
  uint64_t host_pack_min = 64ull << 20;   // the floor of the pack buffers' first guess, in bytes
  // the restart-point search (zs_k_sync_size): a lane started at candidate j stops at candidate j + sync_pass + 1
  uint32_t sync_pass = 8;
};

// ---- the host-buffer entries' pipeline (capi.cpp, host_batch_run)
#define ZS_HOST_CHUNK_STREAMS 64u  // batches of fewer streams run as one chunk whatever their size
// zs_set_option's values of "host_chunk_min" and "host_pack_min"
static inline bool zs_host_chunk_min_ok(int v) { return v >= 0; }
static inline bool zs_host_pack_min_ok(int v) { return v >= 0; }
// The chunks of a host batch of n streams and tin input bytes: streams [bnd[k], bnd[k + 1]), K =
// bnd.size() - 1 of them.  One chunk, or -- from ZS_HOST_CHUNK_STREAMS streams and host_chunk_min bytes
// on -- four, cut at n/8, 4n/8 and 7n/8: the small first chunk starts the kernels early, the small last
// one leaves little to copy back after them.  With n >= 64 no chunk is empty.
static inline void zs_plan_host_chunks(const zs_route_opts& o, uint32_t n, uint64_t tin, std::vector<uint32_t>& bnd) {
  bnd.assign(1, 0u);
  if (o.host_chunk_min && n >= ZS_HOST_CHUNK_STREAMS && tin >= o.host_chunk_min)
    for (uint32_t f : {1u, 4u, 7u}) bnd.push_back((uint32_t)((uint64_t)n * f / 8));
  bnd.push_back(n);
}
// The first size of the packed-output buffers (d_pack, h_out), which hold produced bytes, not
// capacities: four times the input or host_pack_min, whichever is more, and never more than the
// capacities' sum; 16 bytes of slack.  A guess: host_batch_run grows them when a chunk does not fit.
static inline uint64_t zs_plan_host_pack0(const zs_route_opts& o, uint64_t tin, uint64_t tout) {
  return std::min<uint64_t>(tout, std::max<uint64_t>(4 * tin, o.host_pack_min)) + 16;
}

// ---- checksums of long streams
#define ZS_CK_PART_MIN 1024u
#define ZS_CK_PART_MAX (1u << 20)
#define ZS_CK_PARTS_MAX (1u << 24)  // parts of one call at most (a wave each: the grid); past it, one wave per stream
// zs_set_option's values of "checksum_split" and "checksum_part"
static inline bool zs_checksum_split_ok(int v) { return v >= 0; }
static inline bool zs_checksum_part_ok(int v) {
  return v >= (int)ZS_CK_PART_MIN && v <= (int)ZS_CK_PART_MAX && !(v & (v - 1));
}
// A data checksum of n streams: one wave per stream (zs_k_checksum, as ever), or -- with any
// stream's length bound above checksum_split -- a wave per part of checksum_part bytes and a wave
// per stream that joins them (zs_k_checksum_parts, zs_k_checksum_fold).  Stream i then has
// max(1, ceil(len_bound[i] / part)) parts, pfirst[i] .. pfirst[i + 1] of the pstream map.
struct zs_checksum_plan {
  bool split = false;
  uint32_t part_lg = 16;
  uint32_t P = 0;                        // parts in all (0 unsplit)
  std::vector<uint32_t> pfirst, pstream;  // n + 1 and P entries (empty unsplit)
  size_t ws_bytes = 0;                   // the parts' values: 4 bytes each
  // the map behind a metadata block (at a multiple of 256): pfirst, then pstream
  size_t map_pstream() const { return (4ull * pfirst.size() + 255) & ~size_t(255); }
  size_t map_bytes() const { return split ? map_pstream() + ((4ull * P + 255) & ~size_t(255)) : 0; }
};
// len_bound: the lengths where the host knows them (deflate, the checksum entries), the output
// capacities for the inflate check, whose lengths exist only on the device
static inline void zs_plan_checksum(const zs_route_opts& o, uint32_t n, const uint32_t* len_bound,
                                    zs_checksum_plan& p) {
  p.split = false;
  p.P = 0;
  p.ws_bytes = 0;
  p.pfirst.clear();
  p.pstream.clear();
  for (p.part_lg = 0; (1u << p.part_lg) < o.checksum_part;) p.part_lg++;
  uint64_t total = 0;
  bool any = false;
  for (uint32_t i = 0; i < n; i++) {
    any |= o.checksum_split && len_bound[i] > o.checksum_split;
    total += std::max<uint64_t>(1, ((uint64_t)len_bound[i] + o.checksum_part - 1) >> p.part_lg);
  }
  if (!any || total > ZS_CK_PARTS_MAX) return;
  p.split = true;
  p.P = (uint32_t)total;
  p.ws_bytes = 4ull * p.P;
  p.pfirst.resize(n + 1);
  p.pstream.reserve(p.P);
  for (uint32_t i = 0; i < n; i++) {
    p.pfirst[i] = (uint32_t)p.pstream.size();
    const uint64_t k = std::max<uint64_t>(1, ((uint64_t)len_bound[i] + o.checksum_part - 1) >> p.part_lg);
    p.pstream.insert(p.pstream.end(), (size_t)k, i);
  }
  p.pfirst[n] = p.P;
}

// ---- inflate
// A member's span slots in the segmented decode: one per ZS_SEG_BLOCK_BITS input
// bits for the blocks, twice the spans of the narrowest lanes, 8 more; its
// pieces' bound; its u16 scratch elements (each piece 16-byte aligned and padded).
static inline uint64_t zs_seg_spans(uint32_t in_len) {
  const uint64_t nbits = 8ull * in_len;
  return nbits / ZS_SEG_BLOCK_BITS + 2 * nbits / (64ull * ZS_SEG_W) + 8;
}
static inline uint32_t zs_seg_pmax(uint32_t in_len) {
  const uint64_t nbits = 8ull * in_len, spans = zs_seg_spans(in_len);
  // (x 2: split mode cuts pieces in two)
  return 2u * (uint32_t)std::min<uint64_t>(spans * ZS_SEG_LANES, nbits / ZS_SEG_W + spans + 1);
}
static inline uint64_t zs_seg_scratch_elems(uint32_t in_len, uint32_t out_cap) {
  return (((uint64_t)out_cap + 7) & ~7ull) + ZS_SEG_PAD * (uint64_t)zs_seg_pmax(in_len) + 16;
}

// A lane launch: members per workgroup and the root-table instance
// (zs_k_inflate_lane<rt, ..>; narrow workgroups afford per-lane root tables, inflate_lane.hip)
struct zs_lane_launch {
  uint32_t block = 1;
  int rt = 0;
};

struct zs_inflate_plan {
  // the large members (batch indices), by the path that decodes them beside the lane kernel
  std::vector<uint32_t> seg, split, wave;
  uint32_t wave_min = 0;  // the lane kernel skips members that are large by this threshold (0: none)
  zs_lane_launch lane;    // the lane kernel over the whole batch
  uint32_t piece_cap = 0;   // split path: u16 values per piece
  uint64_t val_stride = 0;  // u32 values per split member
  bool wave_refw = false;   // wave list: zs_k_inflate_wave<wave_refw> ...
  bool wave_lanes = false;  // ... or one lane each, zs_k_inflate_lane<wave_lane.rt, true>
  zs_lane_launch wave_lane;
  // Members with a preset dictionary (dict_len[i] != 0), by their route: the single-call
  // ones decode in the lane kernel's dictionary instances (zs_k_inflate_lane<.., .., true>,
  // launched for the whole batch in place of the plain ones), the others in the exact kernel
  std::vector<uint32_t> dict_lane, dict_exact;
  bool dict = false;  // any: the dictionary instances
};

// A dictionary member the lane kernel decodes: one inflate() call of the reference
// decodes it whole (one 32 KiB input sub-chunk, one 64 KiB output buffer,
// streams.ts:6-7,78-93), so with the dictionary in the window (w_next = w_have, or 0
// and a full window) inflate_fast takes only its contiguous window copies
// (inffast.ts:113-126,149-162) and the bytes are zlib's.
ZS_PLAN_FN bool zs_inf_dict_single(uint32_t in_len, uint32_t out_cap) {
  return in_len <= 32768u && out_cap <= 65536u;
}

// Everything inflate_device decides about a batch with the fast path on
// (options o, o.inflate_fast set).  dict_len: the members' dictionary lengths, or
// null for a batch without dictionaries.
static inline void zs_plan_inflate(const zs_route_opts& o, int wbits, uint32_t n, const uint32_t* in_len,
                                   const uint32_t* out_cap, zs_inflate_plan& p, const uint32_t* dict_len = nullptr) {
  // lane-per-member fast path; anything but a clean end of stream goes to the exact kernel.
  // A lane's decode is a dependent chain of loads, so the chip wants many
  // waves more than full ones: up to 16,384 members, thin workgroups (one
  // wave each) until ~4096 waves; above, 1024 waves of up to 64 members.
  // Measured (MI355X): 65,536 members want 64 per workgroup (every lane resident at
  // once, 548 B of LDS each); 8,192 want two (C5-i 29.5 -> 23.7 ms at 8 -> 2: four
  // waves per SIMD hide each other's waits, with little divergence inside each).
  uint32_t B = (uint32_t)o.lane_block;
  if (!B) {
    if (n <= 16384u)
      for (B = 1; B < 64 && (n + B - 1) / B > 4608u;) B <<= 1;  // (~4096 waves; a few members over 8,192 keep two per wave)
    else
      for (B = 64; B > 8 && (n + B - 1) / B < 1024u;) B >>= 1;
  }
  // Large members (more than inflate_wave_min input bytes) decode one per wave
  // on the side stream, beside the lane kernel: one lane would take the
  // batch's whole time on such a member.  The wave kernel tracks the
  // reference's inflate() calls and reproduces their window-wrap copy
  // (inflate_wave.hip, zs_refcalls); the lane kernel skips exactly these members.
  p.wave_min = 0;
  p.seg.clear();
  p.split.clear();
  p.wave.clear();
  // Dictionary members never go to the segmented, split or wave decoders (none of them
  // reads a dictionary): the dictionary lane instance or the exact kernel
  p.dict_lane.clear();
  p.dict_exact.clear();
  for (uint32_t i = 0; dict_len && i < n; i++)
    if (dict_len[i]) (zs_inf_dict_single(in_len[i], out_cap[i]) ? p.dict_lane : p.dict_exact).push_back(i);
  p.dict = !p.dict_lane.empty() || !p.dict_exact.empty();
  // "Large" members decode beside the lane kernel.  With the segmented decode on,
  // a small batch's members are large from seg_small_min bytes on: one lane each
  // would leave most of the chip idle (the per-rank shards of the 8-GPU configs).
  uint32_t big_min = o.inflate_wave_min;
  if (o.inflate_seg && n <= o.seg_small_batch && o.seg_small_min && (!big_min || o.seg_small_min < big_min))
    big_min = o.seg_small_min;
  // Large raw members whose decode carries no call-boundary behaviour
  // (deflate64; raw deflate without the window-wrap copy) are cut at their
  // block boundaries and decoded piecewise (inflate_split.hip); the rest of
  // the large members take the wave kernel.  The pieces' u16 scratch is
  // bounded: members past kSplitScratch take the wave kernel too.
  const bool splittable = o.inflate_split && (wbits == -16 || (wbits == -15 && !o.inflate_ref_wrap));
  p.piece_cap = 0;
  p.val_stride = 0;
  if (big_min) {
    constexpr size_t kSplitScratch = 2ull << 30;
    constexpr uint32_t kPieceCapMax = 4u << 20;  // values per piece
    // the segmented decode's u16 scratch (2 bytes per byte of capacity) is
    // bounded too (option seg_scratch_mb): members past it take the split / wave kernels
    uint64_t seg_bytes = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (!zs_inf_large(in_len[i], out_cap[i], big_min) || (dict_len && dict_len[i])) continue;
      // (the segmented decode keeps bit positions in 32 bits; members with long
      // blocks or long copies -- large deflate64 ones, high expansions -- decode
      // faster with a wave per block / per member, which copies 64 bytes at a time)
      const bool longcopies = zs_inf_expands(in_len[i], out_cap[i]) ||
                              (wbits == -16 && 8ull * in_len[i] > ZS_SEG_SPLIT_BITS);
      if (o.inflate_seg && in_len[i] < (1u << 29) && !longcopies) {
        const uint64_t sb = 2 * zs_seg_scratch_elems(in_len[i], out_cap[i]);
        if (seg_bytes + sb <= o.seg_scratch_max) {
          seg_bytes += sb;
          p.seg.push_back(i);
          continue;
        }
      }
      const uint32_t pc = (std::min(out_cap[i], kPieceCapMax) + 1u) & ~1u;
      const uint32_t npc = std::max(p.piece_cap, pc);
      const uint64_t nvs = std::max<uint64_t>(p.val_stride, (out_cap[i] + 3ull) & ~3ull);
      if (splittable && (2ull * ZS_SPLIT_MAX * npc + 4ull * nvs) * (p.split.size() + 1) <= kSplitScratch) {
        p.split.push_back(i);
        p.piece_cap = npc;
        p.val_stride = nvs;
      } else {
        p.wave.push_back(i);
      }
    }
    if (!p.wave.empty() || !p.split.empty() || !p.seg.empty()) p.wave_min = big_min;
  }
  // Narrow workgroups with large members beside them (side stream): the
  // LDS-canon instance, 68 VGPRs, so the side stream's waves find slots on
  // every SIMD (C5-ii: 34 -> 26 ms); alone, the register instance (C5-i:
  // 24.4 vs 25.7 ms)
  p.lane.block = B;
  p.lane.rt = B > 16 ? 0 : p.wave_min ? 2 : 1;
  // deflate64 never runs inflate_fast in the reference: no window-wrap copy to reproduce
  p.wave_refw = o.inflate_ref_wrap && wbits != -16;
  // Many large members: one lane each (the lane kernel's REFW instance,
  // the reference's calls tracked per lane) -- a wave per member keeps its
  // bookkeeping in scalars, and the waves of a CU share one scalar unit
  // (4,096 x 256 KiB: wave kernel 176 ms)
  const uint32_t nw = (uint32_t)p.wave.size();
  p.wave_lanes = p.wave_refw && o.lane_large_min && nw >= o.lane_large_min;
  for (uint32_t i = 0; p.wave_lanes && i < nw; i++) p.wave_lanes = in_len[p.wave[i]] < (1u << 29);  // 32-bit bit positions
  // thin workgroups to ~4096 waves (4,096 x 256 KiB: one lane per wave 95 ms, two 110, four 144)
  uint32_t B2 = 1;
  while (B2 < 64 && (nw + B2 - 1) / B2 > 4096u) B2 <<= 1;
  p.wave_lane.block = B2;
  p.wave_lane.rt = B2 <= 16 ? 2 : 0;
}

// The segmented decode of the members `list` of a batch (seg_launch): per-member
// prefix arrays, the big members, and the instances and grids of its kernels.
struct zs_seg_plan {
  std::vector<uint32_t> spb, pbase;  // prefix sums per list entry: span slots, pieces
  std::vector<uint64_t> sbase;       // ... and u16 scratch elements
  std::vector<uint32_t> big, big_s;  // members over seg_big_bits input bits: list indices, batch indices
  uint32_t nb = 0;                   // span slots in all
  uint32_t nwalk = 0;                // the walk's grid: one wave per member, ZS_SPLIT_MAX per big one
  bool d64 = false, refw = false;    // zs_k_seg_decode<d64, refw>; the fallback zs_k_inflate_wave<refw>
  bool w2k = false, large = false;   // zs_k_seg_walk<d64, w2k ? 2048 : 1024, large && !d64>
  uint32_t walk_bits = 0;            // its bits-per-lane argument
  int split = 0;
  bool rsmall = false;               // zs_k_seg_resolve<512, 65536> (else <256, 32768>)
  uint32_t gdec = 0, gfb = 0;        // grids of the decode and of the fallback
};

static inline void zs_plan_seg(const zs_route_opts& o, int wbits, const std::vector<uint32_t>& list,
                               const uint32_t* in_len, const uint32_t* out_cap, zs_seg_plan& p) {
  const uint32_t ng = (uint32_t)list.size();
  p.d64 = wbits == -16;
  p.refw = o.inflate_ref_wrap && !p.d64;
  p.pbase.assign(ng + 1, 0);
  p.sbase.assign(ng + 1, 0);
  p.spb.assign(ng + 1, 0);
  p.big.clear();
  p.big_s.clear();
  uint64_t gbits = 0;
  for (uint32_t k = 0; k < ng; k++) {
    const uint32_t i = list[k];
    const uint64_t nbits = 8ull * in_len[i];
    p.spb[k + 1] = p.spb[k] + 2 * (uint32_t)zs_seg_spans(in_len[i]);  // (x 2: split mode)
    p.pbase[k + 1] = p.pbase[k] + zs_seg_pmax(in_len[i]);
    p.sbase[k + 1] = p.sbase[k] + zs_seg_scratch_elems(in_len[i], out_cap[i]);
    // the big members' list indices for the walk, their stream indices for the finder
    if (nbits > o.seg_big_bits) {
      p.big.push_back(k);
      p.big_s.push_back(i);
    }
    gbits += nbits;
  }
  p.nb = p.spb[ng];
  p.nwalk = ng + (uint32_t)p.big.size() * (ZS_SPLIT_MAX - 1u);
  // The sync window: 2048 bits when the walks all fit the chip at once (the 2048-bit
  // instance takes 49 KB of LDS: three per CU) and the members are large (blocks
  // wide enough for lanes of >= 2048 bits), so that fewer neighbours fail to meet
  // (512 x 256 KiB: 5.3 -> 4.2 ms); otherwise 1024 (occupancy: 1,024 x 256 KiB 7.6 vs 6.6 ms)
  p.large = gbits >= 65536ull * 8 * ng;  // members of 64 KiB of input or more on average
  p.w2k = o.seg_wide && p.nwalk <= 3u * o.ncu && p.large;
  // bits per lane: large members (4,096 x 256 KiB: 17.2 -> 15.9 ms, its 512-member shard 3.70 -> 3.57) walk fewer,
  // wider spans; 64 KiB members keep 2048 (the 1,024-member gunzip shard: 2.11 vs 2.45 ms, the decode's pieces
  // too few to fill the chip) -- tools/segbits_ab.sh
  const uint32_t sbits = o.seg_bits ? o.seg_bits : gbits >= (1ull << 19) * ng ? 4096u : 2048u;
  p.walk_bits = std::max<uint32_t>(sbits, p.w2k ? 2048u : 0u);
  // Split mode: the plan cuts each piece in two at the first symbol start past its lane's middle (the walk
  // records it), so the decode runs twice the pieces, each half as long.  The resolve then takes twice the
  // rounds (one piece per round) and the plan twice the steps, so it pays only where the decode of few large
  // members leaves SIMDs idle: a rank's 512 x 256 KiB shard 3.13 -> 2.93 ms (decode 1.36 -> 0.78, plan
  // 0.08 -> 0.20, resolve 0.30 -> 0.50); 1,024 x 256 KiB 5.07 -> 5.52, C5-i's 1,024 x 64 KiB 1.93 -> 2.09
  // (profiles/r06/seg/split_*)
  p.split = o.seg_split == 2 ? (ng <= 2u * o.ncu && p.large ? 1 : 0) : o.seg_split;
  // one wave per span taken, grid-stride over the work list
  p.gdec = std::min<uint32_t>(p.nb, 8192u);
  // the resolve: four members per CU (256 threads, a 32 KiB ring) unless the batch is too small to fill them
  p.rsmall = ng <= 2u * o.ncu;
  // (the members the resolve listed: usually none, so a small grid walks the list)
  p.gfb = std::min<uint32_t>(ng, 256u);
}

// ---- deflate
// The L4..9 parse runs two waves per stream (zs_k_parse_2w: 512-position
// segments, two rounds' speculative passes at once) for a batch of n streams?
// The whole batch decides (chunks of one batch share the scratch layout).
static inline int zs_parse_waves_for(const zs_route_opts& o, uint32_t n) {
  if (o.parse_waves) return o.parse_waves;
  return n < ZS_PARSE2W_AUTO ? 2 : 1;
}
static inline uint32_t zs_parse_seg(int w) {
  return w == 4 ? ZS_PARSE4W_SEG : w == 2 ? ZS_PARSE2W_SEG : ZS_PARSE_SEG;
}
static inline uint32_t zs_parse_seg_words(int w) {
  return w == 4 ? ZS_PARSE4W_SEG_WORDS : w == 2 ? ZS_PARSE2W_SEG_WORDS : ZS_PARSE_SEG_WORDS;
}

// ---- compression strategies (deflateInit2_'s strategy, deflate.ts:289-290; dispatch :923-931)
#define ZS_STRAT_DEFAULT 0
#define ZS_STRAT_FILTERED 1
#define ZS_STRAT_HUFFMAN_ONLY 2
#define ZS_STRAT_RLE 3
#define ZS_STRAT_FIXED 4
// who tallies the symbols of a batch
#define ZS_TALLY_LEVEL 0  // the level's own path: deflate_fast (1..3) or the match search + lazy parse (4..9)
#define ZS_TALLY_HUFF 1   // zs_k_huff_tally: every byte a literal (deflate_huff, deflate.ts:1525-1565)
#define ZS_TALLY_RLE 2    // zs_k_rle_tally: zlib's deflate_rle, matches at distance 1
struct zs_strategy_plan {
  bool stored = false;    // level 0: deflate_stored whatever the strategy (deflate.ts:925)
  int tally = ZS_TALLY_LEVEL;
  bool filtered = false;  // the lazy parse's _filt instances (levels 4..9; deflate_fast has no filtered branch)
  bool fixed = false;     // zs_k_trees takes the static trees' length (trees.ts:567)
  int wrap_strategy = 0;  // zs_k_wrap: >= 2 clears the zlib level bits and sets gzip XFL 4 below level 9 (deflate.ts:757,798)
  int plan_level = 0;     // the level zs_plan_deflate lays the workspace out for (1 for the tallies: no windows, no parse scratch)
};
// level: 0..9; strategy: 0..4 (validated by the caller)
static inline zs_strategy_plan zs_plan_strategy(const zs_route_opts& o, int level, int strategy) {
  zs_strategy_plan sp;
  sp.plan_level = level;
  if (level == 0) {
    sp.stored = true;
    return sp;
  }
  sp.wrap_strategy = strategy;
  if (strategy == ZS_STRAT_FILTERED) sp.filtered = level >= 4;
  else if (strategy == ZS_STRAT_HUFFMAN_ONLY) sp.tally = ZS_TALLY_HUFF;
  else if (strategy == ZS_STRAT_RLE) sp.tally = o.rle_ref ? ZS_TALLY_HUFF : ZS_TALLY_RLE;
  else if (strategy == ZS_STRAT_FIXED) sp.fixed = true;
  if (sp.tally != ZS_TALLY_LEVEL) sp.plan_level = 1;
  return sp;
}
// zs_k_huff_tally's grid: one workgroup per (stream, block of 16,383 bytes); a stream of n
// bytes has n / 16383 + 1 blocks (the last one final, possibly empty)
struct zs_huff_chunk {
  uint32_t s, b;
};
static inline void zs_plan_huff_chunks(uint32_t n, const uint32_t* in_len, std::vector<zs_huff_chunk>& chunks) {
  chunks.clear();
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t b = 0; b <= in_len[i] / ZS_SYM_END; b++) chunks.push_back({i, b});
}

// ---- deflateInit2_'s windowBits and memLevel (deflate.ts:253-343)
// w_bits 9..15 (8 runs as 9, deflate.ts:295-297); hash_bits = memLevel + 7 and hash_shift =
// (hash_bits + 2) / 3 in whole numbers (deflate.ts:312-315; the `<<` of :110 truncates the
// reference's fraction); a block closes after sym_end = lit_bufsize - 1 symbols, lit_bufsize =
// 1 << (memLevel + 6) (deflate.ts:323,336).  The default -- 15 / memLevel 8 -- is what every
// kernel had compiled in before the parameters existed.
struct zs_deflate_params {
  uint32_t w_bits = 15, hash_bits = 15, hash_shift = 5, sym_end = ZS_SYM_END;
  bool is_default() const { return w_bits == 15 && hash_bits == 15 && hash_shift == 5 && sym_end == ZS_SYM_END; }
  uint32_t w_size() const { return 1u << w_bits; }
  zs_kpar kpar() const { return {1u << w_bits, hash_shift, (1u << hash_bits) - 1u, sym_end}; }
};
// window_bits 8..15, mem_level 1..9 (validated by the caller)
static inline zs_deflate_params zs_make_params(int window_bits, int mem_level) {
  zs_deflate_params q;
  q.w_bits = (uint32_t)(window_bits == 8 ? 9 : window_bits);
  q.hash_bits = (uint32_t)mem_level + 7u;
  q.hash_shift = (q.hash_bits + 2u) / 3u;
  q.sym_end = (1u << (mem_level + 6)) - 1u;
  return q;
}
// deflateInit2_'s windowBits argument (deflate.ts:272-294): -9..-15 raw, 8..15 zlib, 25..31
// gzip; -8 and everything else is refused.  Returns the window bits 8..15, or 0.
static inline int zs_wbits_split(int wbits, int* wrap) {
  int w = wbits;
  *wrap = 1;
  if (w < 0) {
    *wrap = 0;
    w = -w;
  } else if (w > 15) {
    *wrap = 2;
    w -= 16;
  }
  if (w == 8 && *wrap != 1) return 0;  // (only a zlib stream takes 8, and runs it as 9: deflate.ts:281-297)
  return w >= 8 && w <= 15 ? w : 0;
}
// Levels 1..3 with non-default parameters (deflate_fast.hip): the kernel instance and its LDS.
// The tables of the reference are head[1 << hash_bits] and prev[w_size], u16 each; beside them
// sits the input ring -- 32 KiB in the group-speculative kernel, w_size bytes in the step-by-step
// one.  memLevel 9 (65,536 heads, 128 KiB) leaves the group kernel no room, and the step-by-step
// one only up to w_bits 13 (128 + 16 + 8 KiB); at w_bits 14 and 15 its head[] lives in a
// per-stream global workspace (128 KiB per stream, resident in L2).
#define ZS_FAST_LDS_MAX (160u << 10)
enum zs_fast_route { ZS_FAST_GROUP = 0, ZS_FAST_SERIAL = 1, ZS_FAST_SERIAL_GHEAD = 2 };
struct zs_fast_plan {
  zs_fast_route route = ZS_FAST_GROUP;
  uint32_t lds_bytes = 0;    // dynamic LDS of the launch
  uint64_t ghead_bytes = 0;  // the global head[] workspace of the whole batch (route ZS_FAST_SERIAL_GHEAD)
};
static inline zs_fast_plan zs_plan_fast_params(const zs_deflate_params& q, bool fast_group, uint32_t n) {
  zs_fast_plan f;
  const uint32_t head = 2u << q.hash_bits, prev = 2u << q.w_bits;
  const uint32_t group = head + prev + 32768u, serial = head + prev + q.w_size();
  if (fast_group && group <= ZS_FAST_LDS_MAX) {
    f.route = ZS_FAST_GROUP;
    f.lds_bytes = group;
  } else if (serial <= ZS_FAST_LDS_MAX) {
    f.route = ZS_FAST_SERIAL;
    f.lds_bytes = serial;
  } else {
    f.route = ZS_FAST_SERIAL_GHEAD;
    f.lds_bytes = prev + q.w_size();
    f.ghead_bytes = (uint64_t)head * n;
  }
  return f;
}

// ---- a deflate request: what an entry point asks for, whichever of the eight it is
struct zs_deflate_req {
  int level = 6;  // 0..9 (-1 has become 6, deflate.ts:268-270); anything else is refused
  int wrap = 0;   // 0 deflate-raw, 1 zlib, 2 gzip; -1: a windowBits the entry does not take
  int strategy = ZS_STRAT_DEFAULT;
  zs_deflate_params q;
  bool dict = false;  // the call carries preset dictionaries (a batch with every length 0 is the plain batch)
  // 0, or ZS_FLUSH_FULL: the call carries Z_FULL_FLUSH positions (a batch without any is the plain batch)
  int flush = 0;
  // with flush: every piece behind the first is PRIMED with the 32 KiB in front of it as a preset dictionary
  // (pigz's construction).  Not one of zlib's flush values: a flag of its own.
  bool primed = false;
  // 0, or the block size 1..ZS_BGZF_BLOCK_MAX of a BGZF call: every stream is cut into
  // pieces of that many bytes, each a finished raw-deflate stream in a gzip frame of its own
  uint32_t bgzf = 0;
};
#define ZS_BGZF_BLOCK_MAX 65280u  // htslib's BGZF_BLOCK_SIZE (0xff00): the input of one block at most
#define ZS_BGZF_HEADER 18u        // the gzip header with the BC subfield ...
#define ZS_BGZF_TRAILER 8u        // ... and crc32 + ISIZE
#define ZS_BGZF_EOF 28u           // the end-of-file block
#define ZS_BGZF_MEMBER_MAX 65536u // BSIZE is 16 bits of (total size - 1)
#define ZS_FLUSH_FULL 3  // Z_FULL_FLUSH, common/constants.ts
// streams + flush points of one device call at most: the segments are the y dimension of the
// trees' and emit's grids
#define ZS_FLUSH_SEG_MAX 65535u
enum zs_deflate_err {
  ZS_DE_OK = 0,
  ZS_DE_WBITS,         // "unsupported windowBits (use -15, 15 or 31)"
  ZS_DE_LEVEL,         // "invalid level"
  ZS_DE_STRATEGY,      // "invalid strategy"
  ZS_DE_WINDOW_BITS,   // "invalid window bits"
  ZS_DE_MEM_LEVEL,     // "invalid memLevel"
  ZS_DE_DICT_ARRAYS,   // "null dictionary arrays"
  ZS_DE_DICT_BUFFER,   // "null dictionary buffer"
  ZS_DE_DICT_GZIP,     // "dictionaries are for deflate-raw (-15) and zlib (15) only"
  ZS_DE_DICT_LEVEL0,   // "level 0 with a preset dictionary is not built"
  ZS_DE_DICT_LONG,     // "stream too long for a preset dictionary"
  ZS_DE_PARAMS_LEVEL0, // "level 0 with non-default windowBits / memLevel is not built"
  ZS_DE_RLE_LONG,      // "stream too long for Z_RLE"
  ZS_DE_ALIGN,         // "output offsets/capacities must be multiples of 4"
  ZS_DE_DICT_COMBINED, // internal (no public entry makes it): dictionaries with a strategy or parameters
  ZS_DE_FLUSH_MODE,    // "flush mode not built"
  ZS_DE_FLUSH_INVALID, // "invalid flush"
  ZS_DE_FLUSH_ARRAYS,  // "null flush arrays"
  ZS_DE_FLUSH_POS,     // "invalid flush positions"
  ZS_DE_FLUSH_LEVEL0,  // "level 0 with a flush point is not built"
  ZS_DE_FLUSH_MANY,    // "too many flush points (streams + flush points above 65,535 in one call)"
  ZS_DE_BGZF_BLOCK,    // "invalid BGZF block size"
  ZS_DE_BGZF_ARRAYS,   // "null arrays"
  ZS_DE_BGZF_MANY,     // "too many BGZF blocks (streams + blocks above 65,535 in one call)"
  ZS_DE_COUNT
};
// The request of the plain, _strategy and _dict entries: wbits -15 / 15 / 31.  Only a strategy out of
// range fails here, before the context is looked at (deflate.ts:289-290).
static inline zs_deflate_err zs_deflate_make_req(int level, int wbits, int strategy, bool dict, zs_deflate_req* r) {
  r->level = level == -1 ? 6 : level;
  r->wrap = wbits == -15 ? 0 : wbits == 15 ? 1 : wbits == 31 ? 2 : -1;
  r->strategy = strategy;
  r->q = zs_deflate_params();
  r->dict = dict;
  return strategy < 0 || strategy > ZS_STRAT_FIXED ? ZS_DE_STRATEGY : ZS_DE_OK;
}
// ... and of the _params entries: deflateInit2_'s windowBits and memLevel (validation deflate.ts:281-294)
static inline zs_deflate_err zs_deflate_make_req_params(int level, int wbits, int mem_level, zs_deflate_req* r) {
  int wrap;
  const int wb = zs_wbits_split(wbits, &wrap);
  if (!wb) return ZS_DE_WINDOW_BITS;
  if (mem_level < 1 || mem_level > 9) return ZS_DE_MEM_LEVEL;
  r->level = level == -1 ? 6 : level;
  r->wrap = wrap;
  r->strategy = ZS_STRAT_DEFAULT;
  r->q = zs_make_params(wb, mem_level);
  r->dict = false;
  return ZS_DE_OK;
}
// ... and of the _flush entries: deflate()'s flush argument (deflate.ts:720: anything outside
// Z_NO_FLUSH .. Z_BLOCK is Z_STREAM_ERROR).  Z_FULL_FLUSH alone is built; a fault is reported before
// the context is looked at.
static inline zs_deflate_err zs_deflate_make_req_flush(int level, int wbits, int flush, zs_deflate_req* r) {
  zs_deflate_make_req(level, wbits, ZS_STRAT_DEFAULT, false, r);
  if (flush == 1 || flush == 2 || flush == 5) return ZS_DE_FLUSH_MODE;  // Z_PARTIAL_FLUSH, Z_SYNC_FLUSH, Z_BLOCK
  if (flush != ZS_FLUSH_FULL) return ZS_DE_FLUSH_INVALID;
  r->flush = flush;
  return ZS_DE_OK;
}
// ... and of the _primed entries: the _flush entries' positions, no flush argument; all three formats
static inline zs_deflate_err zs_deflate_make_req_primed(int level, int wbits, zs_deflate_req* r) {
  zs_deflate_make_req(level, wbits, ZS_STRAT_DEFAULT, false, r);
  r->flush = ZS_FLUSH_FULL;  // (the marker's bytes and the piece rules are the full flush's)
  r->primed = true;
  return ZS_DE_OK;
}
// ... and of the _bgzf entries: gzip members, block_bytes 0 = ZS_BGZF_BLOCK_MAX.  The level's
// fault is named before the block size's, both before the context is looked at.
static inline zs_deflate_err zs_deflate_make_req_bgzf(int level, uint32_t block_bytes, zs_deflate_req* r) {
  zs_deflate_make_req(level, 31, ZS_STRAT_DEFAULT, false, r);
  if (r->level < 0 || r->level > 9) return ZS_DE_LEVEL;
  if (block_bytes > ZS_BGZF_BLOCK_MAX) return ZS_DE_BGZF_BLOCK;
  r->bgzf = block_bytes ? block_bytes : ZS_BGZF_BLOCK_MAX;
  return ZS_DE_OK;
}
// The most a piece of n bytes becomes as a finished raw-deflate stream (zs_deflate_bound(n, -15), deflate.ts:615-674)
ZS_PLAN_FN uint64_t zs_bgzf_piece_bound(uint64_t n) { return n + (n >> 12) + (n >> 14) + (n >> 25) + 7; }
// A full block fits BSIZE's 16 bits, so no piece is ever retried with less input (htslib's loop)
static_assert(ZS_BGZF_BLOCK_MAX + (ZS_BGZF_BLOCK_MAX >> 12) + (ZS_BGZF_BLOCK_MAX >> 14) + (ZS_BGZF_BLOCK_MAX >> 25) + 7 +
                      ZS_BGZF_HEADER + ZS_BGZF_TRAILER <= ZS_BGZF_MEMBER_MAX,
              "a BGZF block of ZS_BGZF_BLOCK_MAX input bytes must fit 65,536 bytes");
// zs_deflate_bound_bgzf: the blocks' bounds and frames, then the end-of-file block.  The stored form of
// level 0 (piece + 5 + 26) is smaller, so one bound serves all levels.
ZS_PLAN_FN uint64_t zs_bgzf_bound(uint64_t source_len, uint32_t block_bytes) {
  const uint64_t B = block_bytes ? block_bytes : ZS_BGZF_BLOCK_MAX;
  if (B > ZS_BGZF_BLOCK_MAX) return 0;
  const uint64_t q = source_len / B, r = source_len % B, fr = ZS_BGZF_HEADER + ZS_BGZF_TRAILER;
  return q * (zs_bgzf_piece_bound(B) + fr) + (r ? zs_bgzf_piece_bound(r) + fr : 0) + ZS_BGZF_EOF;
}
// The data blocks of a stream of len bytes
ZS_PLAN_FN uint64_t zs_bgzf_blocks(uint64_t len, uint32_t B) { return (len + B - 1) / B; }
// The arrays of a call, as far as validation reads them
struct zs_deflate_call {
  uint32_t n = 0;
  const uint32_t* in_len = nullptr;
  const uint64_t* out_off = nullptr;
  const uint32_t* out_cap = nullptr;
  bool caller_regions = false;  // the device entries: the capacities must be multiples of 4 too
  bool dict_arrays = false, dict_buf = false;  // the dictionary offsets and lengths / bytes are given
  const uint32_t* dict_len = nullptr;          // (with dict_arrays)
  // requests with flush set: stream i's flush positions are flush_pos[flush_first[i] .. flush_first[i + 1])
  const uint64_t* flush_first = nullptr;
  const uint32_t* flush_pos = nullptr;
  bool null_arrays = false;  // a _bgzf entry was given n streams and a null offset, length or capacity array
};
// A BGZF call (r.bgzf): its arrays, then streams + data blocks of one device call against the trees' and
// emit's grid limit (as the flush points')
static inline zs_deflate_err zs_deflate_validate_bgzf(const zs_deflate_req& r, const zs_deflate_call& a, bool count) {
  if (!r.bgzf || a.n == 0) return ZS_DE_OK;
  if (a.null_arrays) return ZS_DE_BGZF_ARRAYS;
  if (!count) return ZS_DE_OK;
  uint64_t m = a.n;
  for (uint32_t i = 0; i < a.n; i++) m += zs_bgzf_blocks(a.in_len[i], r.bgzf);
  return m > ZS_FLUSH_SEG_MAX ? ZS_DE_BGZF_MANY : ZS_DE_OK;
}
static inline bool zs_deflate_any_flush(const zs_deflate_req& r, const zs_deflate_call& a) {
  return r.flush && a.n && a.flush_first && a.flush_first[a.n] > a.flush_first[0];
}
// The flush positions of a call: 0 <= p_1 < p_2 < ... <= in_len[i] for every stream (a second flush
// with no input between is Z_BUF_ERROR in the reference, deflate.ts:742-743: refused up front), no
// level 0 (deflate_stored's cuts depend on the output buffers), and at most ZS_FLUSH_SEG_MAX segments.
static inline zs_deflate_err zs_deflate_validate_flush(const zs_deflate_req& r, const zs_deflate_call& a) {
  if (!r.flush || a.n == 0) return ZS_DE_OK;
  if (!a.flush_first) return ZS_DE_FLUSH_ARRAYS;
  const uint64_t* ff = a.flush_first;
  for (uint32_t i = 0; i < a.n; i++)
    if (ff[i + 1] < ff[i]) return ZS_DE_FLUSH_POS;
  if (ff[a.n] == ff[0]) return ZS_DE_OK;
  if (!a.flush_pos) return ZS_DE_FLUSH_ARRAYS;
  for (uint32_t i = 0; i < a.n; i++)
    for (uint64_t k = ff[i]; k < ff[i + 1]; k++)
      if (a.flush_pos[k] > a.in_len[i] || (k > ff[i] && a.flush_pos[k] <= a.flush_pos[k - 1])) return ZS_DE_FLUSH_POS;
  if (r.level == 0) return ZS_DE_FLUSH_LEVEL0;
  if (ff[a.n] - ff[0] + a.n > ZS_FLUSH_SEG_MAX) return ZS_DE_FLUSH_MANY;
  return ZS_DE_OK;
}
static inline bool zs_deflate_any_dict(const zs_deflate_req& r, const zs_deflate_call& a) {
  for (uint32_t i = 0; r.dict && a.dict_len && i < a.n; i++)
    if (a.dict_len[i]) return true;
  return false;
}
// What a host entry checks of the whole batch before it stages anything; an empty batch is done
// after it, whatever its level.  The chunks then pass zs_deflate_validate one by one.
static inline zs_deflate_err zs_deflate_validate_host(const zs_deflate_req& r, const zs_deflate_call& a) {
  if (r.dict && !a.dict_arrays) return ZS_DE_DICT_ARRAYS;
  if (r.bgzf) return zs_deflate_validate_bgzf(r, a, false);  // (the chunks count their own blocks)
  if (r.flush) {  // (no entry takes flush positions and dictionaries): the device batches' order
    if (a.n == 0) return ZS_DE_OK;
    if (r.wrap < 0) return ZS_DE_WBITS;
    if (r.level < 0 || r.level > 9) return ZS_DE_LEVEL;
    return zs_deflate_validate_flush(r, a);
  }
  if (a.n == 0 || !zs_deflate_any_dict(r, a)) return ZS_DE_OK;
  if (!a.dict_buf) return ZS_DE_DICT_BUFFER;
  if (r.wrap == 2) return ZS_DE_DICT_GZIP;  // deflateSetDictionary refuses gzip (deflate.ts:373)
  if (r.level == 0) return ZS_DE_DICT_LEVEL0;
  return ZS_DE_OK;
}
// The first fault of a device batch, in the order the entries have always reported them.
static inline zs_deflate_err zs_deflate_validate(const zs_deflate_req& r, const zs_route_opts& o,
                                                 const zs_deflate_call& a) {
  if (r.wrap < 0) return ZS_DE_WBITS;
  if (r.level < 0 || r.level > 9) return ZS_DE_LEVEL;  // deflate.ts:281-294
  if (r.strategy < 0 || r.strategy > ZS_STRAT_FIXED) return ZS_DE_STRATEGY;
  if (r.dict && a.n) {
    if (!a.dict_arrays) return ZS_DE_DICT_ARRAYS;
    if (zs_deflate_any_dict(r, a)) {
      if (!a.dict_buf) return ZS_DE_DICT_BUFFER;
      if (r.wrap == 2) return ZS_DE_DICT_GZIP;
      if (r.level == 0) return ZS_DE_DICT_LEVEL0;
      if (r.strategy != ZS_STRAT_DEFAULT || !r.q.is_default()) return ZS_DE_DICT_COMBINED;
      for (uint32_t i = 0; i < a.n; i++)
        if (a.dict_len[i] && a.in_len[i] > 0xffffffffu - ZS_W_SIZE) return ZS_DE_DICT_LONG;
    }
  }
  if (a.n == 0) return ZS_DE_OK;
  if (r.bgzf && a.null_arrays) return ZS_DE_BGZF_ARRAYS;
  for (uint32_t i = 0; i < a.n; i++)
    if ((a.out_off[i] & 3) || (a.caller_regions && (a.out_cap[i] & 3))) return ZS_DE_ALIGN;
  if (const zs_deflate_err e = zs_deflate_validate_flush(r, a)) return e;
  if (const zs_deflate_err e = zs_deflate_validate_bgzf(r, a, true)) return e;
  if (r.bgzf) return ZS_DE_OK;  // (level 0 is zs_k_bgzf_stored's, whatever the layer above)
  if (r.level == 0) return r.q.is_default() ? ZS_DE_OK : ZS_DE_PARAMS_LEVEL0;
  if (zs_plan_strategy(o, r.level, r.strategy).tally == ZS_TALLY_RLE)  // (zs_k_rle_tally's 32-bit positions run 4,416 past a stream's end)
    for (uint32_t i = 0; i < a.n; i++)
      if (a.in_len[i] > 0xffff0000u) return ZS_DE_RLE_LONG;
  return ZS_DE_OK;
}

// Device metadata block: in_off | in_len | out_off | out_cap | pos_base | blk_base | the sweep's
// windows; for a deflate batch with preset dictionaries the streams' dictionary offsets, lengths,
// ids and parse starts, the joined streams' offsets and lengths and the distinct dictionaries'
// offsets and lengths (no room without); zs_k_huff_tally's list last.  Every section starts on
// a multiple of 256 bytes.
struct zs_meta_layout {
  size_t in_off, in_len, out_off, out_cap, pos_base, blk_base, segs;
  size_t doff, dlen, did, start, joff, jlen, uoff, ulen;
  size_t chunks, bytes;
  explicit zs_meta_layout(uint32_t n = 0, uint32_t nwin = 0, bool dict = false, uint32_t ndict = 0, size_t nchunks = 0) {
    size_t o = 0;
    auto take = [&](size_t b) { size_t r = o; o = (o + b + 255) & ~size_t(255); return r; };
    const size_t nd = dict ? n : 0, nu = dict ? ndict : 0;
    in_off = take(8ull * n);
    in_len = take(4ull * n);
    out_off = take(8ull * n);
    out_cap = take(4ull * n);
    pos_base = take(8ull * n);
    blk_base = take(4ull * n);
    segs = take(sizeof(zs_sweep_seg) * nwin);  // the sweep's windows (levels 4..9)
    doff = take(8ull * nd);
    dlen = take(4ull * nd);
    did = take(4ull * nd);
    start = take(4ull * nd);
    joff = take(8ull * nd);
    jlen = take(4ull * nd);
    uoff = take(8ull * nu);
    ulen = take(4ull * nu);
    chunks = take(sizeof(zs_huff_chunk) * nchunks);
    bytes = o;
  }
};

// ---- Z_FULL_FLUSH points.  At a full flush with all input consumed the reference
// closes the pending block, writes an empty stored block, clears the hash and sets strstart =
// block_start = insert = 0 (deflate.ts:942-955): the piece behind the point is compressed as a fresh
// stream that starts on a byte boundary.  A stream with k flush points is therefore planned as k + 1
// SEGMENTS, each a stream of its own to every per-position kernel (zs_plan_deflate over the
// segments' lengths); the flushed layout kernels (deflate_flush.hip) put them back together.
struct zs_flush_plan {
  uint32_t n = 0, M = 0;          // streams, segments
  std::vector<uint32_t> sfirst;   // each stream's first segment (sfirst[n] = M)
  std::vector<uint32_t> sstream;  // each segment's stream (sstream[M] = n)
  std::vector<uint32_t> soff;     // each segment's start in its stream ...
  std::vector<uint32_t> slen;     // ... and its length
  // a primed batch (zs_plan_primed; else empty): each segment's prime length and the length of its J
  std::vector<uint32_t> lp, nv;
  std::vector<uint32_t> joff;     // ... and J's start in its stream, soff - lp
};
// flush_first / flush_pos: positions that passed zs_deflate_validate_flush (flush_first may be null: none)
static inline void zs_plan_flush(uint32_t n, const uint32_t* in_len, const uint64_t* flush_first,
                                 const uint32_t* flush_pos, zs_flush_plan& f) {
  f.n = n;
  f.sfirst.assign(n + 1, 0);
  f.sstream.clear();
  f.soff.clear();
  f.slen.clear();
  for (uint32_t i = 0; i < n; i++) {
    f.sfirst[i] = (uint32_t)f.sstream.size();
    uint32_t at = 0;
    for (uint64_t k = flush_first ? flush_first[i] : 0; flush_first && k < flush_first[i + 1]; k++) {
      f.sstream.push_back(i);
      f.soff.push_back(at);
      f.slen.push_back(flush_pos[k] - at);
      at = flush_pos[k];
    }
    f.sstream.push_back(i);  // the piece Z_FINISH closes (empty after a flush at the stream's end)
    f.soff.push_back(at);
    f.slen.push_back(in_len[i] - at);
  }
  f.M = (uint32_t)f.sstream.size();
  f.sfirst[n] = f.M;
  f.sstream.push_back(n);
  f.lp.clear();
  f.nv.clear();
  f.joff.clear();
}
// ---- Primed pieces.  A piece behind a point is compressed against the 32 KiB in front of
// it as a preset dictionary (deflateSetDictionary on a raw stream): the dictionary path's "run on J =
// tail(dict) || data, start the parse at L'" (DESIGN 4.6), where J is a slice of the stream itself:
// segment g of zs_plan_flush gets the prime length lp = min(soff, 32768), J = [soff - lp, soff + slen)
// of its stream and the parse start lp.  zs_plan_deflate then runs over the segments with dict_len = lp.
static inline void zs_plan_primed(zs_flush_plan& f) {
  f.lp.resize(f.M);
  f.nv.resize(f.M);
  f.joff.resize(f.M);
  for (uint32_t g = 0; g < f.M; g++) {
    f.lp[g] = f.soff[g] < ZS_W_SIZE ? f.soff[g] : ZS_W_SIZE;
    f.joff[g] = f.soff[g] - f.lp[g];
    f.nv[g] = f.lp[g] + f.slen[g];  // (at most the stream's length: no overflow)
  }
}
// ---- BGZF: stream i is cut every B bytes into ceil(len / B) segments, each a finished raw
// stream in a gzip frame of its own; an empty stream has none (its output is the end-of-file block alone).
// The maps are zs_plan_flush's, and zs_plan_deflate runs over the segments' lengths without the marker's slot.
static inline void zs_plan_bgzf(uint32_t n, const uint32_t* in_len, uint32_t B, zs_flush_plan& f) {
  f.n = n;
  f.sfirst.assign(n + 1, 0);
  f.sstream.clear();
  f.soff.clear();
  f.slen.clear();
  for (uint32_t i = 0; i < n; i++) {
    f.sfirst[i] = (uint32_t)f.sstream.size();
    for (uint64_t at = 0; at < in_len[i]; at += B) {
      f.sstream.push_back(i);
      f.soff.push_back((uint32_t)at);
      f.slen.push_back((uint32_t)std::min<uint64_t>(B, in_len[i] - at));
    }
  }
  f.M = (uint32_t)f.sstream.size();
  f.sfirst[n] = f.M;
  f.sstream.push_back(n);
}
// The flushed batch's section of the metadata block, behind the segments' own (zs_meta_layout of
// M): the streams' arrays and the two maps; and the scan workspace of the layout kernels.
#define ZS_FLUSH_TILE 256u  // segments per workgroup of the layout scan
struct zs_flush_layout {
  size_t in_off, in_len, out_off, out_cap, sfirst, sstream, bytes;
  size_t scan_bytes;  // u64 per segment (+ 1), then u64 per tile
  uint32_t tiles;
  zs_flush_layout(size_t base, uint32_t n, uint32_t M) {
    size_t o = base;
    auto take = [&](size_t b) { size_t r = o; o = (o + b + 255) & ~size_t(255); return r; };
    in_off = take(8ull * n);
    in_len = take(4ull * n);
    out_off = take(8ull * n);
    out_cap = take(4ull * n);
    sfirst = take(4ull * (n + 1));
    sstream = take(4ull * (M + 1));
    bytes = o;
    tiles = M / ZS_FLUSH_TILE + 1;  // (M + 1 entries)
    scan_bytes = 8ull * (M + 1) + 8ull * tiles;
  }
};

// deflate.ts:86-103: good_length, max_lazy, nice_length, max_chain of levels 0..9
static const zs_level_cfg zs_level_cfgs[10] = {{0, 0, 0, 0},     {4, 4, 8, 4},     {4, 5, 16, 8},     {4, 6, 32, 32},
                                               {4, 4, 16, 16},   {8, 16, 32, 32},  {8, 16, 128, 128}, {8, 32, 128, 256},
                                               {32, 128, 258, 1024}, {32, 258, 258, 4096}};

// Who finds the matches of a batch, who tallies its symbols, and which build of those kernels
enum zs_match_route {
  ZS_MATCH_NONE = 0,  // nobody: the tallies, and levels 1..3 (deflate_fast finds its own)
  ZS_MATCH_SWEEP,     // zs_k_bucket + zs_k_sweep over the windows
  ZS_MATCH_CHAIN      // the chain-walk kernels zs_k_prev + zs_k_match
};
enum zs_sym_route {
  ZS_SYM_HUFF = 0,          // zs_k_huff_tally
  ZS_SYM_RLE,               // zs_k_rle_tally
  ZS_SYM_PARSE,             // the lazy parse, levels 4..9
  ZS_SYM_FAST_GROUP,        // levels 1..3: zs_k_fast, the group-speculative replay
  ZS_SYM_FAST_SERIAL,       // ... the step-by-step one
  ZS_SYM_FAST_SERIAL_GHEAD  // ... with head[] in the global workspace
};
enum zs_variant {
  ZS_VAR_PLAIN = 0,
  ZS_VAR_PAR,   // the *_par instances: non-default windowBits / memLevel
  ZS_VAR_DICT,  // the _dict / DICT instances: joined streams
  ZS_VAR_FILT   // the lazy parse's _filt instances (Z_FILTERED at levels 4..9)
};

// Everything the host layer decides about a deflate batch: the workspace layout, the routes, the
// kernel instances' coordinates, the grids and the metadata block.  With the sweep (levels
// 4..9, option match_sweep), every stream is cut into WINDOWS of at most 65,535
// inserted positions: a stream of up to 65,537 bytes is one; a longer one has a
// first window owning positions [0, 65520) and then windows owning 32,752
// positions each after a 32,768-position look-back (more than MAX_DIST: every
// candidate of an own position is in its window).
struct zs_deflate_plan {
  std::vector<uint64_t> pos;       // each stream's base in the per-position tables (8-aligned)
  std::vector<uint32_t> blk;       // ... and in the block records
  std::vector<zs_sweep_seg> segs;  // the sweep's windows (batch stream indices); empty without the sweep
  std::vector<uint32_t> win0;      // each stream's first window (win0[n] = the total)
  // Members: u16 per position for a stream of one window (pos); 65,536 per window after them for longer ones
  uint64_t P = 0, members = 0;
  uint32_t B = 0, max_len = 0, max_blk = 0;
  int pw = 1;  // waves per stream of the parse (zs_k_parse / _2w / _4w)
  bool sweep = false;  // levels 4..9: zs_k_bucket + zs_k_sweep (else the chain-walk kernels zs_k_prev + zs_k_match)
  // A batch with preset dictionaries (else empty / 0): each stream's parse start L' in its
  // joined stream, the joined streams' offsets in the join buffer, and that buffer's bytes
  std::vector<uint32_t> start;
  std::vector<uint64_t> joff;
  uint64_t J = 0;
  size_t prevd_bytes = 0, mres_bytes = 0, syms_bytes = 0, pscr_bytes = 0, codes_bytes = 0, hdr_bytes = 0;
  // ---- the launch
  zs_deflate_req req;   // what was asked (level and wrap go to the wrapper kernels, q to the *_par ones)
  uint32_t n = 0;
  bool stored = false;  // level 0: zs_k_stored alone, whatever the strategy; nothing below is set
  zs_match_route match = ZS_MATCH_NONE;
  zs_sym_route sym = ZS_SYM_PARSE;
  zs_variant variant = ZS_VAR_PLAIN;
  int cfg = 0;          // index into zs_level_cfgs
  int nice_bucket = 2;  // zs_k_fast<NW, ..>: 2, 4 or 8 by the level's nice_length
  bool lane_order = true;  // the ORD instances of zs_k_bucket, zs_k_prev and zs_k_fast
  bool sweep_u8 = false;   // zs_k_sweep<true> (zs_sweep_uniform8 of the level's chain)
  bool fixed = false;      // zs_k_trees takes the static trees' length (Z_FIXED)
  int wrap_strategy = 0;   // zs_k_wrap's strategy argument
  bool dict = false;       // the streams are joined streams; the dictionary sections of ml are laid out
  uint32_t ndict = 0;      // ... and this many distinct dictionaries
  // grids: per stream in workgroups of 256 lanes; zs_k_match's, zs_k_dict_join's and zs_k_stored's x
  // (y: the streams); the others are n, segs.size(), chunks.size() and (max_blk, n)
  uint32_t g_streams = 0, g_match_x = 0, g_join_x = 0, g_stored_x = 0;
  uint32_t fast_lds = 0;     // dynamic LDS of the levels 1..3 kernel
  uint64_t ghead_bytes = 0;  // its global head[] workspace (ZS_SYM_FAST_SERIAL_GHEAD)
  std::vector<zs_huff_chunk> chunks;  // zs_k_huff_tally's (stream, block) list
  zs_meta_layout ml;
};

// The part of a preset dictionary that enters the window (deflate.ts:383-392: its last w_size bytes)
ZS_PLAN_FN uint32_t zs_dict_tail(uint32_t dict_len) { return dict_len < ZS_W_SIZE ? dict_len : ZS_W_SIZE; }

// r: a request that passed zs_deflate_validate.  fast_group, lane_order: the context's options of
// those names.  dict_len: the streams' preset-dictionary lengths (r.dict), or null for a batch
// without dictionaries, and ndict the number of distinct ones (zs_dict_distinct).  A stream with a
// dictionary is planned as its JOINED stream -- the
// dictionary's tail of L' = zs_dict_tail bytes, then the data: the
// per-position tables, the windows and max_len follow nv = L' + n, the windows'
// own positions start at L' (p.start), the block records follow n.
// r.q: deflateInit2_'s windowBits / memLevel.  Non-default ones take the chain-walk kernels at
// levels 4..9 (zs_k_prev + zs_k_match follow prev[] links whatever the hash; the sweep's
// signatures rest on the 15-bit hash, deflate_sweep.hip:24-27), and the block records follow
// sym_end: a stream of n bytes closes at most n / sym_end + 1 blocks.
static inline void zs_plan_deflate(const zs_deflate_req& r, const zs_route_opts& o, bool fast_group, bool lane_order,
                                   uint32_t n, const uint32_t* in_len, const uint32_t* dict_len, uint32_t ndict,
                                   zs_deflate_plan& p) {
  const zs_strategy_plan sp = zs_plan_strategy(o, r.level, r.strategy);
  const zs_deflate_params& q = r.q;
  if (!r.dict && !r.primed) dict_len = nullptr;  // (a primed batch's are the segments' prime lengths)
  p.req = r;
  p.n = n;
  p.stored = sp.stored;
  p.dict = dict_len != nullptr;
  p.ndict = p.dict ? ndict : 0;
  p.g_streams = (n + 255) / 256;
  p.segs.clear();
  p.win0.clear();
  p.chunks.clear();
  p.start.clear();
  p.joff.clear();
  p.members = p.J = 0;
  p.sweep = false;
  p.pscr_bytes = 0;
  p.fast_lds = 0;
  p.ghead_bytes = 0;
  if (sp.stored) {
    // level 0: 256 threads x 16 bytes per workgroup over the longest stream's stored blocks and wrapper
    uint64_t max_total = 0;
    for (uint32_t i = 0; i < n; i++) {
      const uint64_t t = (r.wrap == 0 ? 0 : r.wrap == 1 ? 6 : 18) + 5ull * (in_len[i] / ZS_STORED_CHUNK + 1) + in_len[i];
      max_total = std::max(max_total, t);
    }
    p.g_stored_x = (uint32_t)((max_total + 4095) / 4096);
    p.ml = zs_meta_layout(n);
    return;
  }
  const int level = sp.plan_level;  // (1 for the tallies: no windows, no parse scratch)
  const bool par = !q.is_default();
  const bool sweep = level >= 4 && o.match_sweep && !par;
  p.sweep = sweep;
  p.pos.resize(n);
  p.blk.resize(n);
  p.P = 0;
  p.B = p.max_len = p.max_blk = 0;
  if (dict_len) {
    p.start.resize(n);
    p.joff.resize(n);
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t lp = dict_len ? zs_dict_tail(dict_len[i]) : 0u;
    const uint64_t nv = (uint64_t)lp + in_len[i];
    if (dict_len) {
      p.start[i] = lp;
      p.joff[i] = p.J;
      p.J += (nv + 15) & ~15ull;  // joined streams start 16-aligned (the sweep's 16-byte window loads)
    }
    p.pos[i] = p.P;
    p.P += (nv + 7) & ~7ull;  // per-position tables start 8-aligned (16-B link loads in zs_k_match)
    p.blk[i] = p.B;
    const uint32_t nb = in_len[i] / q.sym_end + 2 + (r.flush ? 1u : 0u);  // (a flushed segment's marker block)
    p.B += nb;
    p.max_len = std::max(p.max_len, (uint32_t)std::min<uint64_t>(nv, 0xffffffffull));
    p.max_blk = std::max(p.max_blk, nb);
  }
  if (sweep) {
    uint64_t mb = (p.P + 7) & ~7ull;
    p.win0.resize(n + 1);
    for (uint32_t i = 0; i < n; i++) {
      p.win0[i] = (uint32_t)p.segs.size();
      const uint32_t lp = dict_len ? p.start[i] : 0u;  // the first window's own positions start behind the dictionary
      const uint32_t len = lp + in_len[i];
      if (len <= 65537u) {
        p.segs.push_back({i, 0u, lp, len, p.pos[i], 0});
        continue;
      }
      for (uint64_t lo = 0; lo < len; mb += 65536) {
        const uint32_t base = lo == 0 ? 0u : (uint32_t)lo - 32768u;
        p.segs.push_back({i, base, lo == 0 ? lp : (uint32_t)lo - base, lo == 0 ? ZS_SEG_FIRST : 32768u + ZS_SEG_OWN, mb, 0});
        lo += lo == 0 ? ZS_SEG_FIRST : ZS_SEG_OWN;
      }
    }
    p.win0[n] = (uint32_t)p.segs.size();
    p.members = mb;
  }
  p.pw = level >= 4 ? zs_parse_waves_for(o, n) : 1;
  p.prevd_bytes = 2 * std::max(p.members, p.P) + 128;
  p.mres_bytes = 8 * p.P + 64;
  p.syms_bytes = 4 * (p.P + n) + 64;
  p.pscr_bytes = level >= 4 ? 4ull * zs_parse_seg_words(p.pw) * (p.P / zs_parse_seg(p.pw) + n + 1) : 0;
  p.codes_bytes = 4ull * (ZS_L_CODES + ZS_D_CODES) * p.B;
  p.hdr_bytes = 4ull * ZS_HDR_WORDS * p.B;
  // the routes and the instances
  const zs_level_cfg& cfg = zs_level_cfgs[r.level];
  p.cfg = r.level;
  p.variant = par ? ZS_VAR_PAR : p.dict ? ZS_VAR_DICT : sp.filtered ? ZS_VAR_FILT : ZS_VAR_PLAIN;
  p.fixed = sp.fixed;
  p.wrap_strategy = sp.wrap_strategy;
  p.lane_order = lane_order;
  p.nice_bucket = cfg.nice <= 8 ? 2 : cfg.nice <= 16 ? 4 : 8;
  p.sweep_u8 = zs_sweep_uniform8(cfg.chain) != 0;
  p.g_match_x = (p.max_len + 8191) / 8192;
  p.g_join_x = std::max(1u, (uint32_t)(((uint64_t)p.max_len + 4095) / 4096));  // the joined streams: 4 KiB per workgroup
  if (sp.tally != ZS_TALLY_LEVEL) {
    p.match = ZS_MATCH_NONE;
    p.sym = sp.tally == ZS_TALLY_HUFF ? ZS_SYM_HUFF : ZS_SYM_RLE;
    if (sp.tally == ZS_TALLY_HUFF) zs_plan_huff_chunks(n, in_len, p.chunks);
  } else if (level >= 4) {
    p.match = sweep ? ZS_MATCH_SWEEP : ZS_MATCH_CHAIN;
    p.sym = ZS_SYM_PARSE;
  } else {
    // levels 1..3: the instance and its LDS by the tables' sizes; the default parameters fit both kernels
    const zs_fast_plan f = zs_plan_fast_params(q, fast_group, n);
    p.match = ZS_MATCH_NONE;
    p.sym = f.route == ZS_FAST_GROUP ? ZS_SYM_FAST_GROUP : f.route == ZS_FAST_SERIAL ? ZS_SYM_FAST_SERIAL : ZS_SYM_FAST_SERIAL_GHEAD;
    p.fast_lds = f.lds_bytes;
    p.ghead_bytes = f.ghead_bytes;
  }
  p.ml = zs_meta_layout(n, (uint32_t)p.segs.size(), p.dict, p.ndict, p.chunks.size());
}

// ---- an inflate call: the arrays of a plain or _dict entry as far as validation reads them, its
// faults and the order they win in (the restart entries have zs_restart_validate below)
struct zs_inflate_call {
  uint32_t n = 0;
  const uint64_t* out_off = nullptr;  // (may be null: the host entries stage their own regions)
  const uint32_t* out_cap = nullptr;
  bool caller_regions = false;  // the device entries: the capacities must be multiples of 4 too
  bool dict = false;            // a _dict entry (a batch with every length 0 is the plain batch)
  bool dict_arrays = false, dict_buf = false;  // the dictionary offsets and lengths / bytes are given
  const uint32_t* dict_len = nullptr;          // (with dict_arrays)
};
enum zs_inflate_err {
  ZS_IE_OK = 0,
  ZS_IE_CONTEXT,      // "null context"
  ZS_IE_WBITS,        // "unsupported windowBits (use -15, 15, 31 or -16)"
  ZS_IE_DICT_ARRAYS,  // "null dictionary arrays"
  ZS_IE_DICT_BUFFER,  // "null dictionary buffer"
  ZS_IE_DICT_FORMAT,  // "dictionaries are for deflate-raw (-15) and zlib (15) only"
  ZS_IE_ALIGN,        // "output offsets/capacities must be multiples of 4"
  ZS_IE_COUNT
};
static inline const char* zs_inflate_err_text(zs_inflate_err e) {
  static const char* const kMsg[ZS_IE_COUNT] = {
      "",
      "null context",
      "unsupported windowBits (use -15, 15, 31 or -16)",
      "null dictionary arrays",
      "null dictionary buffer",
      "dictionaries are for deflate-raw (-15) and zlib (15) only",
      "output offsets/capacities must be multiples of 4",
  };
  return kMsg[e];
}
static inline bool zs_inflate_any_dict(const zs_inflate_call& a) {
  for (uint32_t i = 0; a.dict && a.dict_len && i < a.n; i++)
    if (a.dict_len[i]) return true;
  return false;
}
// The first fault of a device batch, in the order the entries have always reported them: the format
// (inflateInit2_ / inflateReset2, inflate.ts:138-192) even of an empty batch; the dictionaries -- gzip
// is never in DICT mode (inflateSetDictionary returns Z_STREAM_ERROR, inflate.ts:1229), the 64 KiB
// window of deflate64 is not covered; the alignment last (the decoders store whole dwords).
// ctx: the entry was given a context.
static inline zs_inflate_err zs_inflate_validate(bool ctx, int wbits, const zs_inflate_call& a) {
  if (!ctx) return ZS_IE_CONTEXT;
  if (!(wbits == -15 || wbits == 15 || wbits == 31 || wbits == -16)) return ZS_IE_WBITS;
  if (a.dict && a.n) {
    if (!a.dict_arrays) return ZS_IE_DICT_ARRAYS;
    if (zs_inflate_any_dict(a)) {
      if (!a.dict_buf) return ZS_IE_DICT_BUFFER;
      if (wbits == 31 || wbits == -16) return ZS_IE_DICT_FORMAT;
    }
  }
  for (uint32_t i = 0; i < a.n; i++)
    if ((a.out_off && (a.out_off[i] & 3)) || (a.caller_regions && (a.out_cap[i] & 3))) return ZS_IE_ALIGN;
  return ZS_IE_OK;
}
// What a host entry decides of the whole batch before it stages anything.  An empty batch is done
// whatever its windowBits; the _dict entry wants its arrays even then, and names a dictionary's
// faults before the format's.
static inline zs_inflate_err zs_inflate_validate_host(bool ctx, int wbits, const zs_inflate_call& a) {
  if (!ctx) return ZS_IE_CONTEXT;
  if (a.dict && !a.dict_arrays) return ZS_IE_DICT_ARRAYS;
  if (a.n == 0) return ZS_IE_OK;
  if (zs_inflate_any_dict(a)) {
    if (!a.dict_buf) return ZS_IE_DICT_BUFFER;
    if (wbits == 31 || wbits == -16) return ZS_IE_DICT_FORMAT;
  }
  return zs_inflate_validate(true, wbits, a);
}
// A host entry's device regions: the caller's capacity rounded up to whole words (the kernels store
// dwords); the caller's exact capacities stay the Z_BUF_ERROR limits
static inline uint32_t zs_host_region_cap(uint32_t out_cap) {
  return (uint32_t)std::min<uint64_t>(0xfffffffcull, ((uint64_t)out_cap + 3) & ~3ull);
}

// ---- inflate with restart points (inflateSync, inflate.ts:1267-1337).  Behind a full-flush
// marker the bit stream is byte-aligned and the window empty, so the piece from one restart point to
// the next is a raw deflate stream of its own but for its end: it closes with the marker's empty stored
// block, BFINAL clear.  A stream given with k points is therefore planned as k SEGMENTS; each is copied
// into a gather buffer with the empty final static block 03 00 appended (the last one ends by itself),
// the copies decode as the members of one raw batch (zs_plan_inflate over their lengths, unchanged),
// and the stitch kernel joins their results per stream (inflate_restart.hip).
//
// Segments of one device call at most: every decoder and the stitch run a 64-thread workgroup per
// member, and a launch takes fewer than 2^32 threads.
#define ZS_RESTART_SEG_MAX 67108863u  // (2^32 - 1) / 64
#define ZS_RESTART_MIN_GAP 5u         // a marker alone: three header bits padded to a byte, 00 00 FF FF
#define ZS_RESTART_TILE 4096u         // bytes per workgroup step of the gather and place kernels
enum zs_restart_err {
  ZS_RE_OK = 0,
  ZS_RE_WBITS,      // "unsupported windowBits (use -15, 15 or 31)"
  ZS_RE_D64,        // "deflate64 has no restart points"
  ZS_RE_ARRAYS,     // "null restart arrays"
  ZS_RE_NO_FIRST,   // "a stream without its first point"
  ZS_RE_MANY,       // "too many restart points (more than 67,108,863 segments in one call)"
  ZS_RE_FIRST_OUT,  // "the first point's out_pos must be 0"
  ZS_RE_IN_POS,     // "restart in_pos must increase by at least 5"
  ZS_RE_OUT_POS,    // "restart out_pos must not decrease"
  ZS_RE_PAST_END,   // "restart in_pos past the stream's input"
  ZS_RE_ALIGN,      // "output offsets/capacities must be multiples of 4"
  ZS_RE_COUNT
};
static inline const char* zs_restart_err_text(zs_restart_err e) {
  static const char* const kMsg[ZS_RE_COUNT] = {
      "",
      "unsupported windowBits (use -15, 15 or 31)",
      "deflate64 has no restart points",
      "null restart arrays",
      "a stream without its first point",
      "too many restart points (more than 67,108,863 segments in one call)",
      "the first point's out_pos must be 0",
      "restart in_pos must increase by at least 5",
      "restart out_pos must not decrease",
      "restart in_pos past the stream's input",
      "output offsets/capacities must be multiples of 4",
  };
  return kMsg[e];
}
struct zs_restart_call {
  uint32_t n = 0;
  const uint32_t* in_len = nullptr;
  const uint64_t* out_off = nullptr;  // (may be null: the host entries stage their own regions)
  const uint32_t* out_cap = nullptr;
  bool caller_regions = false;  // the device entry: offsets and capacities are multiples of 4
  // stream i's points are (rin[k], rout[k]), k in rfirst[i] .. rfirst[i + 1]
  const uint64_t* rfirst = nullptr;
  const uint32_t* rin = nullptr;
  const uint32_t* rout = nullptr;
};
// The fault that wins, in this order: the format; the arrays; the index (every stream has its first
// point); the segment count; then the points stream by stream and point by point (out_pos of the
// first, the step of in_pos, the step of out_pos, in_pos against the input's length); the device
// entry's alignment rule last.  Nothing here looks at a context.
static inline zs_restart_err zs_restart_validate(int wbits, const zs_restart_call& a) {
  if (wbits == -16) return ZS_RE_D64;
  if (!(wbits == -15 || wbits == 15 || wbits == 31)) return ZS_RE_WBITS;
  if (a.n == 0) return ZS_RE_OK;
  if (!a.rfirst || !a.rin || !a.rout) return ZS_RE_ARRAYS;
  for (uint32_t i = 0; i < a.n; i++)
    if (a.rfirst[i + 1] <= a.rfirst[i]) return ZS_RE_NO_FIRST;
  if (a.rfirst[a.n] - a.rfirst[0] > ZS_RESTART_SEG_MAX) return ZS_RE_MANY;
  for (uint32_t i = 0; i < a.n; i++)
    for (uint64_t k = a.rfirst[i]; k < a.rfirst[i + 1]; k++) {
      if (k == a.rfirst[i]) {
        if (a.rout[k] != 0) return ZS_RE_FIRST_OUT;
      } else {
        if ((uint64_t)a.rin[k] < (uint64_t)a.rin[k - 1] + ZS_RESTART_MIN_GAP) return ZS_RE_IN_POS;
        if (a.rout[k] < a.rout[k - 1]) return ZS_RE_OUT_POS;
      }
      if (a.rin[k] > a.in_len[i]) return ZS_RE_PAST_END;
    }
  for (uint32_t i = 0; a.out_off && i < a.n; i++)
    if ((a.out_off[i] & 3) || (a.caller_regions && (a.out_cap[i] & 3))) return ZS_RE_ALIGN;
  return ZS_RE_OK;
}

// The length of the wrapper's header in front of the deflate data: 0 raw, 2 zlib; gzip the fixed 10
// bytes plus FEXTRA / FNAME / FCOMMENT / FHCRC (inflate.ts:600-728), or 0 when the magic, the method
// or a reserved flag is wrong or the header does not end inside the n bytes.  FHCRC is skipped, not verified.
ZS_PLAN_FN uint32_t zs_wrapper_header_len_of(int wbits, const uint8_t* p, uint32_t n) {
  if (wbits < 0) return 0;
  if (wbits <= 15) return 2;
  if (!p || n < 10 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xe0)) return 0;
  const uint32_t flg = p[3];
  uint64_t at = 10;
  if (flg & 4) {  // FEXTRA: a 16-bit length, then the field
    if (at + 2 > n) return 0;
    at += 2ull + p[at] + ((uint32_t)p[at + 1] << 8);
    if (at > n) return 0;
  }
  for (uint32_t f = 8; f <= 16; f <<= 1)  // FNAME, FCOMMENT: to a zero byte
    if (flg & f) {
      while (at < n && p[at]) at++;
      if (at >= n) return 0;
      at++;
    }
  if (flg & 2) at += 2;  // FHCRC
  return at <= n ? (uint32_t)at : 0u;
}
// ... and whether the header in front of the first point `at` is well formed and ends exactly there
ZS_PLAN_FN bool zs_wrapper_header_ok(int wbits, const uint8_t* p, uint32_t n, uint32_t at) {
  if (wbits < 0) return at == 0;
  if (wbits <= 15) {  // inflate.ts:560-597: method 8, CINFO <= 7, the check mod 31, no FDICT
    if (at != 2 || n < 2) return false;
    const uint32_t cmf = p[0], flg = p[1];
    return (cmf & 15u) == 8u && (cmf >> 4) <= 7u && ((cmf << 8) + flg) % 31u == 0u && !(flg & 0x20u);
  }
  return at != 0 && zs_wrapper_header_len_of(wbits, p, n) == at;
}

// The PIECES of a call's streams that decode as the members of one batch and are joined per stream: a
// restart call's segments, a gzip file's members, the blocks of a BGZF range.  A planner calls begin, then
// stream by stream rfirst[i] = M and push for each of the stream's pieces, then end.
struct zs_pieces {
  uint32_t n = 0, M = 0;          // streams, pieces
  bool in_place = true;           // every piece's out_pos is a multiple of 4: the pieces decode where they belong
  std::vector<uint32_t> rfirst;   // each stream's first piece (rfirst[n] = M)
  std::vector<uint32_t> rstream;  // each piece's stream
  std::vector<uint32_t> soff, slen;  // the piece's bytes in its stream's input
  std::vector<uint32_t> opos;     // its first byte in its stream's output
  std::vector<uint32_t> ocap;     // its capacity
  std::vector<uint64_t> stoff;    // staging route: its 4-aligned region in the staging buffer
  std::vector<uint32_t> ptile;    // M + 1: prefix sums of the place's tiles
  uint64_t stage_bytes = 0;
  void begin(uint32_t streams) {
    n = streams;
    M = 0;
    in_place = true;
    stage_bytes = 0;
    rfirst.assign(n + 1, 0);
    for (auto* v : {&rstream, &soff, &slen, &opos, &ocap}) v->clear();
    stoff.clear();
    ptile.assign(1, 0);
  }
  // `placed`: the bytes the place kernel moves from staging (the capacity; a range's delivered bytes)
  void push(uint32_t i, uint32_t off, uint32_t len, uint64_t out, uint32_t cap, uint32_t placed) {
    if (M > rfirst[i] && (out & 3u)) in_place = false;
    rstream.push_back(i);
    soff.push_back(off);
    slen.push_back(len);
    opos.push_back((uint32_t)out);
    ocap.push_back(cap);
    stoff.push_back(stage_bytes);
    stage_bytes += ((uint64_t)cap + 3) & ~3ull;
    // (the place's words: the destination's leading bytes of its first word count too)
    ptile.push_back(ptile.back() + (uint32_t)(((uint64_t)placed + 3 + ZS_RESTART_TILE - 1) / ZS_RESTART_TILE));
    M++;
  }
  void end(bool staged = false) {  // staged: never in place, whatever the positions are
    rfirst[n] = M;
    if (staged) in_place = false;
    stage_bytes = in_place ? 0 : stage_bytes + 16;
  }
};
// A section of a metadata block, written on the host and uploaded in one copy: put appends `bytes` from p
// (null: zeros) and returns their offset; every array starts on a multiple of 256 bytes, and so ends the section.
static inline size_t zs_section_put(std::vector<uint8_t>& h, const void* p, size_t bytes) {
  const size_t at = h.size();
  h.resize((at + bytes + 255) & ~size_t(255), 0);
  if (p && bytes) memcpy(h.data() + at, p, bytes);
  return at;
}

struct zs_restart_plan : zs_pieces {  // ocap: olen, cut at the stream's out_cap
  std::vector<uint64_t> goff;     // the segment's copy's place in the gather buffer (a multiple of 16)
  std::vector<uint32_t> glen;     // ... and length: slen + 2 (03 00) unless it is its stream's last
  std::vector<uint32_t> olen;     // the bytes it must produce (the last one: its capacity)
  std::vector<uint32_t> over;     // per stream: the last out_pos lies past out_cap (the capacity outcome)
  std::vector<uint32_t> gtile;    // M + 1: prefix sums of the gather's tiles
  uint64_t gather_bytes = 0;
};
// points that passed zs_restart_validate
static inline void zs_plan_restart(uint32_t n, const uint32_t* in_len, const uint32_t* out_cap, const uint64_t* rfirst,
                                   const uint32_t* rin, const uint32_t* rout, zs_restart_plan& p) {
  p.begin(n);
  p.over.assign(n, 0);
  p.glen.clear();
  p.olen.clear();
  p.goff.clear();
  p.gtile.assign(1, 0);
  uint64_t g = 0;
  for (uint32_t i = 0; i < n; i++) {
    p.rfirst[i] = p.M;
    for (uint64_t k = rfirst[i]; k < rfirst[i + 1]; k++) {
      const bool last = k + 1 == rfirst[i + 1];
      const uint32_t len = (last ? in_len[i] : rin[k + 1]) - rin[k];
      const uint32_t room = out_cap[i] > rout[k] ? out_cap[i] - rout[k] : 0u;
      const uint32_t want = last ? room : rout[k + 1] - rout[k];
      const uint32_t cap = std::min(want, room);
      if (last) p.over[i] = rout[k] > out_cap[i];
      p.push(i, rin[k], len, rout[k], cap, cap);
      p.glen.push_back(last ? len : len + 2);
      p.goff.push_back(g);
      g += ((uint64_t)p.glen.back() + 15) & ~15ull;  // (03 00, then zeros: the readers load whole aligned words)
      p.olen.push_back(want);
      p.gtile.push_back(p.gtile.back() + (uint32_t)(((uint64_t)p.glen.back() + ZS_RESTART_TILE - 1) / ZS_RESTART_TILE));
    }
  }
  p.end();
  p.gather_bytes = g + 16;
}

// ---- inflate that finds its own restart points (inflateSync / syncsearch,
// inflate.ts:1267-1337).  zs_k_sync_scan lists every offset behind the bytes 00 00 FF FF (the
// CANDIDATES: a stored block may hold the same bytes), zs_k_sync_size decodes from the first point
// and from every candidate without storing (one lane per START, zs_sync.h) and records how and
// where each lane ended, the bytes it produced and how far its copies reach back before its start;
// zs_plan_sync follows the records from the first point and emits the points in the restart
// entries' layout, which restart_batch then decodes unchanged.
#define ZS_SYNC_TILE 4096u   // bytes per workgroup step of the scan: 256 lanes, one aligned 16-byte unit each
#define ZS_SYNC_LANES 16u    // starts per workgroup of the size decode (their Huffman state: 2,148 bytes of LDS each)
#define ZS_BGZF_THREADS 256u  // starts per workgroup of the BGZF sizing (inflate_bgzf.hip) ...
#define ZS_BGZF_SLOTS 4u      // ... and the Huffman states a wave of it owns for its starts that must decode
static inline bool zs_sync_pass_ok(int v) { return v >= 1 && v <= 64; }  // zs_set_option's values of "sync_pass"
// how a lane of zs_k_sync_size ended
#define ZS_SYNC_LANDED 1u  // a block closed at a byte boundary behind the marker: `end` is a candidate
#define ZS_SYNC_FINAL 2u   // the final block closed: `end` = the bytes consumed
#define ZS_SYNC_ERROR 3u   // the bytes are no deflate data, or the input is exhausted
#define ZS_SYNC_PASSED 4u  // the work bound: the lane reached candidate j + sync_pass + 1 of its stream
struct zs_sync_rec {
  uint32_t how, end;  // ZS_SYNC_*; the byte offset in the stream's input
  uint32_t len;       // bytes produced up to there
  uint32_t reach;     // the largest (distance - bytes produced so far) over the lane's copies, 0: none positive
};
enum zs_sync_err {
  ZS_SE_OK = 0,
  ZS_SE_WBITS,  // "unsupported windowBits (use -15, 15 or 31)"
  ZS_SE_D64,    // "deflate64 has no restart points"
  ZS_SE_CAPS,   // "restart points are found with given capacities only"
  ZS_SE_ALIGN,  // "output offsets/capacities must be multiples of 4"
  ZS_SE_COUNT
};
static inline const char* zs_sync_err_text(zs_sync_err e) {
  static const char* const kMsg[ZS_SE_COUNT] = {
      "",
      "unsupported windowBits (use -15, 15 or 31)",
      "deflate64 has no restart points",
      "restart points are found with given capacities only",
      "output offsets/capacities must be multiples of 4",
  };
  return kMsg[e];
}
// The fault that wins, in the restart entries' order without their index: the format, even of an
// empty batch; the capacities; the device entry's alignment rule last.  Nothing here looks at a context.
static inline zs_sync_err zs_sync_validate(int wbits, const zs_inflate_call& a) {
  if (wbits == -16) return ZS_SE_D64;
  if (!(wbits == -15 || wbits == 15 || wbits == 31)) return ZS_SE_WBITS;
  if (a.n == 0) return ZS_SE_OK;
  if (!a.out_cap) return ZS_SE_CAPS;
  for (uint32_t i = 0; a.out_off && i < a.n; i++)
    if ((a.out_off[i] & 3) || (a.caller_regions && (a.out_cap[i] & 3))) return ZS_SE_ALIGN;
  return ZS_SE_OK;
}
// candidates plus streams of one call: every one becomes a lane and may become a segment
static inline bool zs_sync_count_ok(uint32_t n, uint64_t candidates) { return candidates + n <= ZS_RESTART_SEG_MAX; }
// The scan's tiles: stream i lies `sh16[i]` bytes into its first aligned 16-byte unit; stile: n + 1 prefix sums
static inline void zs_plan_sync_tiles(uint32_t n, const uint32_t* in_len, const uint32_t* sh16, std::vector<uint32_t>& stile) {
  stile.assign(1, 0u);
  for (uint32_t i = 0; i < n; i++)
    stile.push_back(stile.back() + (in_len[i] ? (uint32_t)(((uint64_t)sh16[i] + in_len[i] + ZS_SYNC_TILE - 1) / ZS_SYNC_TILE) : 0u));
}
struct zs_sync_plan {
  std::vector<uint64_t> rfirst;    // n + 1
  std::vector<uint32_t> rin, rout;  // the points, every stream's first included
  // the chains that end at a PASSED lane behind the first point: the stream, the lane's start and its record's
  // index.  The record's reach covers the tail only up to the bound: the caller sizes the tail to its end
  // (zs_k_sync_tail), raises the record's reach to the whole tail's and plans again.
  std::vector<uint32_t> tstream, tstart;
  std::vector<uint64_t> trec;
};
// Stream i has the first point first[i] (the wrapper's header length, cut at in_len[i]: a header that
// does not fit fails its check in the restart path), the candidates cand[cfirst[i] .. cfirst[i + 1])
// in increasing order, the record rec[i] of the lane started at its first point and rec[n + k] of
// the lane started at candidate k.
//   1. the chain: from the first point, a LANDED lane's end is the next point (a candidate, found by
//      binary search; the chain also stops where it is none, or where the output passes 2^32 - 1)
//   2. the chain's last lane is FINAL, or its start is the last point and the rest of the stream one
//      tail segment, which the restart path decodes or fails as any last segment (a PASSED lane's
//      record knows the tail's reach only up to its bound: see zs_sync_plan's tstream)
//   3. a point behind which the window is not empty (Z_SYNC_FLUSH, Z_PARTIAL_FLUSH) goes: a segment
//      with reach > 0 loses its own point and every earlier kept point that its reach extends past
//      (a stack); the first point is never dropped
//   4. out_pos: the prefix sums of the chain's lengths
// The result passes zs_restart_validate by construction.
static inline void zs_plan_sync(uint32_t n, const uint32_t* in_len, const uint32_t* first, const uint64_t* cfirst,
                                const uint32_t* cand, const zs_sync_rec* rec, zs_sync_plan& p) {
  p.rfirst.assign(1, 0);
  p.rin.clear();
  p.rout.clear();
  p.tstream.clear();
  p.tstart.clear();
  p.trec.clear();
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* c0 = cand + cfirst[i];
    const uint32_t* c1 = cand + cfirst[i + 1];
    const size_t base = p.rin.size();  // the stream's first point: the bottom of the stack
    uint32_t pos = std::min(first[i], in_len[i]);
    uint64_t out = 0;
    const zs_sync_rec* r = &rec[i];
    for (;;) {
      if (p.rin.size() == base || r->reach == 0) {
        p.rin.push_back(pos);
        p.rout.push_back((uint32_t)out);
      } else {
        // this segment's copies read output from out - reach on: every point behind that byte goes too
        const uint64_t low = out > r->reach ? out - r->reach : 0;
        while (p.rin.size() > base + 1 && p.rout.back() > low) {
          p.rin.pop_back();
          p.rout.pop_back();
        }
      }
      if (r->how == ZS_SYNC_PASSED && r != &rec[i]) {  // (the first point is never dropped: its reach decides nothing)
        p.tstream.push_back(i);
        p.tstart.push_back(pos);
        p.trec.push_back((uint64_t)(r - rec));
      }
      if (r->how != ZS_SYNC_LANDED || (uint64_t)r->end < (uint64_t)pos + ZS_RESTART_MIN_GAP || r->end > in_len[i] ||
          out + r->len > 0xffffffffull)
        break;
      const uint32_t* at = std::lower_bound(c0, c1, r->end);
      if (at == c1 || *at != r->end) break;
      pos = r->end;
      out += r->len;
      r = &rec[n + (size_t)(at - cand)];
    }
    p.rfirst.push_back(p.rin.size());
  }
}

// ---- multi-member gzip (zlib's gz_look, gzread.c: behind a member's trailer another member
// starts where the bytes 1f 8b follow).  A stream's members are found like restart points: zs_k_members_scan
// lists every offset q >= 1 whose four bytes pass zs_member_magic (the CANDIDATES: compressed data and
// stored blocks hold the same bytes), zs_k_members_size sizes one member from offset 0 and from every
// candidate without storing (zs_members.h; zs_sync_rec: how, the offset behind the trailer, the bytes
// produced), zs_plan_members follows the records from 0 and lays the members out as the members of ONE
// gzip batch on the caller's own input -- every member ends at its own final block, so nothing is copied.
enum zs_members_err {
  ZS_ME_OK = 0,
  ZS_ME_WBITS,  // "members are a gzip notion (use windowBits 31)"
  ZS_ME_CAPS,   // "members are found with given capacities only"
  ZS_ME_ALIGN,  // "output offsets/capacities must be multiples of 4"
  ZS_ME_COUNT
};
static inline const char* zs_members_err_text(zs_members_err e) {
  static const char* const kMsg[ZS_ME_COUNT] = {
      "",
      "members are a gzip notion (use windowBits 31)",
      "members are found with given capacities only",
      "output offsets/capacities must be multiples of 4",
  };
  return kMsg[e];
}
// The fault that wins: the format, even of an empty batch; the capacities; the device entry's
// alignment rule last.  Nothing here looks at a context.
static inline zs_members_err zs_members_validate(int wbits, const zs_inflate_call& a) {
  if (wbits != 31) return ZS_ME_WBITS;
  if (a.n == 0) return ZS_ME_OK;
  if (!a.out_cap) return ZS_ME_CAPS;
  for (uint32_t i = 0; a.out_off && i < a.n; i++)
    if ((a.out_off[i] & 3) || (a.caller_regions && (a.out_cap[i] & 3))) return ZS_ME_ALIGN;
  return ZS_ME_OK;
}
// the four-byte test of a member's start: the magic, the method, no reserved flag
ZS_PLAN_FN bool zs_member_magic(const uint8_t* p) { return p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && !(p[3] & 0xe0); }

// soff, slen: the last member of a failing chain reaches to the stream's end; ocap: the bytes a member
// produces, 0 where those pass out_cap, the room where unknown
struct zs_members_plan : zs_pieces {
  // the starts whose lane its work bound stopped (ZS_SYNC_PASSED): the stream, the start and its record's
  // index.  The stream's members are planned up to there; the caller sizes these starts to the stream's
  // end (zs_k_members_tail), replaces the records and plans again, until no start is left.
  std::vector<uint32_t> tstream, tstart;
  std::vector<uint64_t> trec;
};
// Stream i has the candidates cand[cfirst[i] .. cfirst[i + 1]) in increasing order, the record rec[i] of
// the lane started at 0 and rec[n + k] of the lane started at candidate k.  From 0:
//   FINAL   a member; it fits when out_pos + len <= out_cap[i] (64-bit: a total above 2^32 - 1 never fits).
//           The first member that does not fit gets no room and ends the list: the decoder reports the
//           capacity outcome for it.  The next start is the member's end, if that is a candidate (found by
//           binary search: the scan's rule IS the test of a member's start); else the stream ends there.
//   ERROR   the stream's last member, with the input to the stream's end and the room that is left, so
//           that the decoder reports the exact error
//   PASSED  a true member that holds more than sync_pass false candidates: on the tail list
// Offset 0 is a member whatever its bytes are (the plain entry's outcome for a stream that is no gzip).
static inline void zs_plan_members(uint32_t n, const uint32_t* in_len, const uint32_t* out_cap, const uint64_t* cfirst,
                                   const uint32_t* cand, const zs_sync_rec* rec, zs_members_plan& p) {
  p.begin(n);
  p.tstream.clear();
  p.tstart.clear();
  p.trec.clear();
  auto member = [&](uint32_t i, uint32_t at, uint32_t len, uint64_t out, uint32_t cap) { p.push(i, at, len, out, cap, cap); };
  for (uint32_t i = 0; i < n; i++) {
    p.rfirst[i] = p.M;
    const uint32_t* c0 = cand + cfirst[i];
    const uint32_t* c1 = cand + cfirst[i + 1];
    uint32_t pos = 0;
    uint64_t out = 0;
    const zs_sync_rec* r = &rec[i];
    for (;;) {
      if (r->how == ZS_SYNC_PASSED) {
        p.tstream.push_back(i);
        p.tstart.push_back(pos);
        p.trec.push_back((uint64_t)(r - rec));
        break;  // (the plan is complete, every stream with a member, once no start is listed)
      }
      if (r->how != ZS_SYNC_FINAL || r->end <= pos || r->end > in_len[i]) {
        member(i, pos, in_len[i] - pos, out, out_cap[i] > out ? (uint32_t)(out_cap[i] - out) : 0u);
        break;
      }
      if (out + r->len > out_cap[i]) {
        member(i, pos, r->end - pos, out, 0u);
        break;
      }
      member(i, pos, r->end - pos, out, r->len);
      out += r->len;
      pos = r->end;
      const uint32_t* at = std::lower_bound(c0, c1, pos);
      if (at == c1 || *at != pos) break;
      r = &rec[n + (size_t)(at - cand)];
    }
  }
  p.end();
}

// The _bgzf entries' flags over a finished plan.  rtrusted: one byte per record, in the
// records' order, set where the record came from a header that was trusted (zs_bgzf.h) and not from the
// data.  trusted[g] is set when planned member g came from such a record and was given the record's full
// len for room: its room is its header's ISIZE, so a capacity outcome of its decode is the header's lie
// and not the caller's capacity.  Not set for the member that got no room because the stream's out_cap is
// passed.  Returns the count of flags set.
static inline uint32_t zs_plan_bgzf_trusted(const zs_members_plan& p, const uint32_t* out_cap, const uint64_t* cfirst,
                                            const uint32_t* cand, const zs_sync_rec* rec, const uint8_t* rtrusted,
                                            std::vector<uint8_t>& trusted) {
  trusted.assign(p.M, 0);
  uint32_t count = 0;
  for (uint32_t g = 0; g < p.M; g++) {
    const uint32_t i = p.rstream[g], at = p.soff[g];
    size_t x = i;  // the member's record: offset 0's, or its candidate's (every planned start behind 0 is one)
    if (at) {
      const uint32_t* c0 = cand + cfirst[i];
      const uint32_t* c1 = cand + cfirst[i + 1];
      const uint32_t* f = std::lower_bound(c0, c1, at);
      if (f == c1 || *f != at) continue;
      x = p.n + (size_t)(f - cand);
    }
    const zs_sync_rec& r = rec[x];
    if (!rtrusted[x] || r.how != ZS_SYNC_FINAL || r.end != at + p.slen[g]) continue;
    if ((uint64_t)p.opos[g] + r.len > out_cap[i] || p.ocap[g] != r.len) continue;
    trusted[g] = 1;
    count++;
  }
  return count;
}

// ---- BGZF ranges by virtual offset (the SAM specification, section 4.1.1: a virtual offset is
// coffset << 16 | uoffset).  Stream i with the range (vb, ve): cb, ub = vb >> 16, vb & 0xffff and ce, ue
// likewise.  The blocks with a start in [cb, ce), and the block at ce when ue > 0, decode whole into staging;
// the place kernel drops ub bytes of the first and keeps ue of the last.
enum zs_bgzf_range_err {
  ZS_BR_OK = 0,
  ZS_BR_ARRAYS,    // "null virtual offset arrays"
  ZS_BR_ORDER,     // "a range's begin lies behind its end"
  ZS_BR_PAST_END,  // "a range's end lies past the stream's input"
  ZS_BR_COUNT
};
static inline const char* zs_bgzf_range_err_text(zs_bgzf_range_err e) {
  static const char* const kMsg[ZS_BR_COUNT] = {
      "",
      "null virtual offset arrays",
      "a range's begin lies behind its end",
      "a range's end lies past the stream's input",
  };
  return kMsg[e];
}
// The fault that wins, behind zs_members_validate's: the arrays, then stream by stream the order and the end.
static inline zs_bgzf_range_err zs_bgzf_range_validate(uint32_t n, const uint32_t* in_len, const uint64_t* vb,
                                                       const uint64_t* ve) {
  if (n == 0) return ZS_BR_OK;
  if (!vb || !ve) return ZS_BR_ARRAYS;
  for (uint32_t i = 0; i < n; i++) {
    if (vb[i] > ve[i]) return ZS_BR_ORDER;
    if ((ve[i] >> 16) > in_len[i]) return ZS_BR_PAST_END;
  }
  return ZS_BR_OK;
}
// The SLICE of a stream of n bytes that the range (vb, ve) reads (vb <= ve, ve >> 16 <= n): from cb to ce when
// ue is 0 -- the block at ce is neither needed nor looked at -- else to the end of the largest block that can
// start at ce, cut at the stream's end.
ZS_PLAN_FN void zs_bgzf_range_slice(uint32_t n, uint64_t vb, uint64_t ve, uint32_t& off, uint32_t& len) {
  const uint64_t cb = vb >> 16, ce = ve >> 16;
  const uint64_t end = (ve & 0xffffu) ? (ce + ZS_BGZF_MEMBER_MAX < n ? ce + ZS_BGZF_MEMBER_MAX : n) : ce;
  off = (uint32_t)cb;
  len = (uint32_t)(end - cb);
}

#define ZS_BGZF_RANGE_MEMBERS 0u  // the stream has members: the stitch reads their results
#define ZS_BGZF_RANGE_EMPTY 1u    // nothing to decode: Z_STREAM_END, out_len 0, consumed = cb
#define ZS_BGZF_RANGE_CHAIN 2u    // the headers fail the stream: Z_DATA_ERROR, ZS_MSG_BGZF_RANGE, consumed = the start
// soff: in the STREAM's input (cb + the block's offset in the slice); ocap: the block's room in staging, its
// ISIZE, 0 for the one the stream's out_cap cuts; opos: where its delivered bytes begin.  Never in place.
struct zs_bgzf_range_plan : zs_pieces {
  std::vector<uint32_t> skip, take;  // bytes dropped in front, bytes delivered
  std::vector<uint8_t> trusted;   // its room is its header's ISIZE (zs_k_members_stitch's flag)
  std::vector<uint32_t> verdict, vcons;  // per stream: ZS_BGZF_RANGE_*, and consumed for the two decided here
};
// Stream i's slice (zs_bgzf_range_slice) was scanned and sized as a stream of its own: cand[cfirst[i] ..
// cfirst[i + 1]) are its candidates, offsets IN THE SLICE in increasing order; rec[i] / rtrusted[i] belong to
// the slice's offset 0 and rec[n + k] / rtrusted[n + k] to candidate k (zs_k_bgzf_size's).  A start counts only
// when its header was trusted.  The chain from 0 follows the records' ends while the start lies in front of
// ce - cb and must land there exactly; with ue > 0 the block at ce is needed too.  Members behind the needed end
// are dropped whatever their records say.  A stream the headers fail -- an untrusted start on the chain, a step
// over ce, ub or ue above its block's ISIZE -- contributes no member.  The first member whose delivered bytes
// pass out_cap gets no room and ends the stream's list: the decoder reports the capacity outcome for it.
static inline void zs_plan_bgzf_range(uint32_t n, const uint32_t* out_cap, const uint64_t* vb, const uint64_t* ve,
                                      const uint64_t* cfirst, const uint32_t* cand, const zs_sync_rec* rec,
                                      const uint8_t* rtrusted, zs_bgzf_range_plan& p) {
  p.begin(n);
  p.skip.clear();
  p.take.clear();
  p.trusted.clear();
  p.verdict.assign(n, ZS_BGZF_RANGE_MEMBERS);
  p.vcons.assign(n, 0);
  struct blk { uint32_t at, end, isize; };
  std::vector<blk> chain;
  for (uint32_t i = 0; i < n; i++) {
    p.rfirst[i] = p.M;
    const uint32_t cb = (uint32_t)(vb[i] >> 16), rce = (uint32_t)((ve[i] >> 16) - (vb[i] >> 16));
    const uint32_t ub = (uint32_t)(vb[i] & 0xffffu), ue = (uint32_t)(ve[i] & 0xffffu);
    const uint32_t* c0 = cand + cfirst[i];
    const uint32_t* c1 = cand + cfirst[i + 1];
    // the trusted record of the start at `pos` of the slice, or null
    auto record = [&](uint32_t pos) -> const zs_sync_rec* {
      size_t x = i;
      if (pos) {
        const uint32_t* f = std::lower_bound(c0, c1, pos);
        if (f == c1 || *f != pos) return nullptr;
        x = n + (size_t)(f - cand);
      }
      return rtrusted[x] && rec[x].how == ZS_SYNC_FINAL && rec[x].end > pos ? &rec[x] : nullptr;
    };
    auto fail = [&](uint32_t pos) {
      p.verdict[i] = ZS_BGZF_RANGE_CHAIN;
      p.vcons[i] = cb + pos;
    };
    chain.clear();
    uint32_t pos = 0;
    bool ok = true;
    for (;;) {
      const bool last = pos == rce;  // (a step over ce fails below: pos never passes it)
      if (last && !ue) break;
      const zs_sync_rec* r = record(pos);
      if (!r || (!last && r->end > rce) || (pos == 0 && ub > r->len) || (last && ue > r->len)) {
        fail(pos);
        ok = false;
        break;
      }
      chain.push_back({pos, r->end, r->len});
      if (last) break;
      pos = r->end;
    }
    if (!ok) continue;
    if (chain.empty()) {  // (cb == ce and ue == 0, so ub == 0 too)
      p.verdict[i] = ZS_BGZF_RANGE_EMPTY;
      p.vcons[i] = cb;
      continue;
    }
    uint64_t out = 0;
    for (size_t k = 0; k < chain.size(); k++) {
      const blk& b = chain[k];
      const uint32_t skip = k == 0 ? ub : 0u;
      const uint32_t upto = (b.at == rce && ue) ? ue : b.isize;  // (the block at ce is on the chain only when ue > 0)
      const uint32_t take = upto - skip;
      const bool fits = out + take <= out_cap[i];
      const uint32_t room = fits ? b.isize : 0u;
      p.push(i, cb + b.at, b.end - b.at, out, room, fits ? take : 0u);
      p.skip.push_back(skip);
      p.take.push_back(take);
      p.trusted.push_back(fits ? 1 : 0);
      if (!fits) break;
      out += take;
    }
  }
  p.end(true);
}

#endif
