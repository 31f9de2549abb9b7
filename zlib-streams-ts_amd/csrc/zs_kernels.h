// zs_kernels.h -- kernel entry points and the batch descriptor shared by the
// HIP translation units and the C-ABI host layer (capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_plan.h"  // zs_sweep_seg, the windows' and the parse segments' sizes

// Per-block record written by the parse / tree kernels.
struct zs_block {
  uint32_t sym_start;   // first symbol (index into the stream's symbol array)
  uint32_t sym_count;
  uint32_t in_start;    // input byte range covered by the block
  uint32_t in_end;
  uint32_t type;        // 0 stored, 1 static, 2 dynamic (trees.ts:574-583)
  uint32_t hdr_bits;    // dynamic-tree header bits (send_all_trees)
  uint32_t data_bits;   // symbol bits incl. END_BLOCK
  uint32_t last;        // bit 0: final block; bit 1: block began before the slid window (reference would copy from a negative index)
  uint32_t pad;
  uint64_t bit_off;     // bit offset of the 3-bit block header in the stream output
  uint64_t bit_end;     // bit offset just past the block (before the final byte pad)
};

// Per-stream record.
struct zs_stream {
  uint32_t nsym;
  uint32_t nblk;
  uint64_t total_bits;  // deflate payload bits (after the wrapper header)
  uint32_t out_len;     // bytes incl. wrapper
  int32_t status;       // Z_STREAM_END / Z_BUF_ERROR
  uint32_t check;       // adler32 / crc32 of the input (wrappers)
  uint32_t pad;
};

// ORD: same-address LDS atomics of one instruction apply in lane order (zs_selftest); false: the ballot form
template <bool ORD>
__global__ void zs_k_prev(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* pos_base,
                          uint16_t* prevd, uint32_t min_len);
__global__ void zs_k_match(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* pos_base,
                           const uint16_t* prevd, uint2* mres, int chain, int nice, uint32_t min_len);
// zs_k_bucket's workgroup: wave 0 claims, the others scatter (a multiple of 64 dividing 16384: the scan's slices)
#define ZS_BK_THREADS 512u
template <bool ORD>
__global__ void zs_k_bucket(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* pos_base,
                            const zs_sweep_seg* segs, uint16_t* members, uint2* mres);
// U8: zs_sweep_uniform8(chain) holds -- the instance whose groups after the opening one are all eight steps
template <bool U8>
__global__ void zs_k_sweep(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* pos_base,
                           const zs_sweep_seg* segs, const uint16_t* members, uint2* mres, int chain, int nice);
// ---- the *_par instances for non-default windowBits / memLevel (zs_par.h: the same sources
// compiled a second time with kp, deflate.ts:295-336, in place of the constants); the kernels
// above and below keep 15 / memLevel 8 compiled in
template <bool ORD>
__global__ void zs_k_prev_par(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                              const uint64_t* pos_base, uint16_t* prevd, uint32_t min_len, zs_kpar kp);
__global__ void zs_k_match_par(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                               const uint64_t* pos_base, const uint16_t* prevd, uint2* mres, int chain, int nice,
                               uint32_t min_len, zs_kpar kp);
#define ZS_PARSE_PAR_DECL(name)                                                                                    \
  __global__ void name##_par(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,                    \
                             const uint64_t* pos_base, const uint32_t* blk_base, const uint2* mres, uint32_t* syms, \
                             zs_block* blocks, zs_stream* streams, uint32_t* scratch, int good, int lazy, zs_kpar kp);
ZS_PARSE_PAR_DECL(zs_k_parse)
ZS_PARSE_PAR_DECL(zs_k_parse_2w)
ZS_PARSE_PAR_DECL(zs_k_parse_4w)
// (DICT = false alone is built; dstart is null)
template <int NW, bool ORD, bool DICT>
__global__ void zs_k_fast_par(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                              const uint64_t* pos_base, const uint32_t* blk_base, uint32_t* syms, zs_block* blocks,
                              zs_stream* streams, int chain, int lazy, int nice, const uint32_t* dstart, zs_kpar kp);
// GH: head[] in the global workspace ghead, 1 << hash_bits u16 per stream (zs_plan_fast_params)
template <bool DICT, bool GH>
__global__ void zs_k_fast_serial_par(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                     const uint64_t* pos_base, const uint32_t* blk_base, uint32_t* syms,
                                     zs_block* blocks, zs_stream* streams, int chain, int lazy, int nice,
                                     const uint32_t* dstart, zs_kpar kp, uint16_t* ghead);
// a block that began before the slid window is never stored (deflate.ts:1120-1124)
__global__ void zs_k_trees_par(const uint8_t* in, const uint64_t* in_off, const uint64_t* pos_base,
                               const uint32_t* blk_base, const uint32_t* syms, zs_block* blocks,
                               const zs_stream* streams, uint32_t* codes, uint32_t* hdr, int nstreams, int fixed);
// the zlib header's CINFO = w_bits - 8 (deflate.ts:754)
__global__ void zs_k_wrap_par(const zs_stream* streams, uint8_t* out, const uint64_t* out_off, const uint32_t* in_len,
                              int wrap, int level, int nstreams, int strategy, uint32_t w_bits);
// the lazy parse (deflate_parse.hip): pass A stages 32 match-table entries per lane in LDS; the
// _dict instances parse joined streams (dictionary tail + data) from dstart[s] on; the _filt
// instances are Z_FILTERED's (a new match of at most 5 bytes is dropped, deflate.ts:1381-1387)
#define ZS_PARSE_DECL(name)                                                                                        \
  __global__ void name(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* pos_base, \
                       const uint32_t* blk_base, const uint2* mres, uint32_t* syms, zs_block* blocks,              \
                       zs_stream* streams, uint32_t* scratch, int good, int lazy);                                 \
  __global__ void name##_dict(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,                   \
                              const uint64_t* pos_base, const uint32_t* blk_base, const uint2* mres, uint32_t* syms, \
                              zs_block* blocks, zs_stream* streams, uint32_t* scratch, int good, int lazy,         \
                              const uint32_t* dstart);                                                           \
  __global__ void name##_filt(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,                   \
                              const uint64_t* pos_base, const uint32_t* blk_base, const uint2* mres, uint32_t* syms, \
                              zs_block* blocks, zs_stream* streams, uint32_t* scratch, int good, int lazy);
ZS_PARSE_DECL(zs_k_parse)
ZS_PARSE_DECL(zs_k_parse_2w)  // two waves per stream, ZS_PARSE2W_SEG-position segments
ZS_PARSE_DECL(zs_k_parse_4w)  // four waves per stream, ZS_PARSE4W_SEG-position segments
// DICT: joined streams (dictionary tail + data): the positions below dstart[s] are inserted, the
// parse starts there; else dstart is unused (null)
template <int NW, bool ORD, bool DICT>
__global__ void zs_k_fast(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint64_t* pos_base,
                          const uint32_t* blk_base, uint32_t* syms, zs_block* blocks, zs_stream* streams, int chain,
                          int lazy, int nice, const uint32_t* dstart);
template <bool DICT>
__global__ void zs_k_fast_serial(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                 const uint64_t* pos_base, const uint32_t* blk_base, uint32_t* syms, zs_block* blocks,
                                 zs_stream* streams, int chain, int lazy, int nice, const uint32_t* dstart);
// A batch with preset dictionaries: stream s's joined stream at joined + joff[s] is the last
// dstart[s] bytes of its dictionary (dict + dict_off[s], dict_len[s] bytes), then its data
__global__ void zs_k_dict_join(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint8_t* dict,
                               const uint64_t* dict_off, const uint32_t* dict_len, const uint32_t* dstart,
                               uint8_t* joined, const uint64_t* joff);
// fixed: Z_FIXED (trees.ts:567: the static trees' length is taken whatever the dynamic ones')
__global__ void zs_k_trees(const uint8_t* in, const uint64_t* in_off, const uint64_t* pos_base, const uint32_t* blk_base,
                           const uint32_t* syms, zs_block* blocks, const zs_stream* streams, uint32_t* codes,
                           uint32_t* hdr, int nstreams, int fixed);
// the tallies of Z_HUFFMAN_ONLY and of zlib's Z_RLE (deflate_strategy.hip): symbols, block records, nsym / nblk
__global__ void zs_k_huff_tally(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                const uint64_t* pos_base, const uint32_t* blk_base, const zs_huff_chunk* chunks,
                                uint32_t* syms, zs_block* blocks, zs_stream* streams);
__global__ void zs_k_rle_tally(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                               const uint64_t* pos_base, const uint32_t* blk_base, uint32_t* syms, zs_block* blocks,
                               zs_stream* streams);
__global__ void zs_k_layout(const uint32_t* blk_base, zs_block* blocks, zs_stream* streams, const uint32_t* out_cap,
                            uint8_t* out, const uint64_t* out_off, int wrap, int nstreams);
// zlib streams with a preset dictionary (dstart[s] != 0): FDICT and DICTID (deflate.ts:767-778)
__global__ void zs_k_layout_dict(const uint32_t* blk_base, zs_block* blocks, zs_stream* streams, const uint32_t* out_cap,
                                 uint8_t* out, const uint64_t* out_off, int wrap, int nstreams, const uint32_t* dstart);
__global__ void zs_k_wrap_dict(const zs_stream* streams, uint8_t* out, const uint64_t* out_off, const uint32_t* in_len,
                               int wrap, int level, int nstreams, const uint32_t* dstart, const uint32_t* did,
                               const uint32_t* dadler);
// a batch with Z_FULL_FLUSH points (deflate_flush.hip): the layout per segment, a scan of the
// segments' bytes over workgroups of ZS_FLUSH_TILE, the blocks rebased to their streams' outputs
__global__ void zs_k_flush_local(const uint32_t* blk_base, zs_block* blocks, zs_stream* segs, const uint32_t* sfirst,
                                 const uint32_t* sstream, zs_stream* streams, uint64_t* segx, uint64_t* tile, uint32_t M);
__global__ void zs_k_flush_tiles(uint64_t* tile, uint32_t T);
__global__ void zs_k_flush_place(const uint32_t* blk_base, zs_block* blocks, zs_stream* segs, const uint32_t* sfirst,
                                 const uint32_t* sstream, zs_stream* streams, const uint64_t* segx, const uint64_t* tile,
                                 const uint32_t* out_cap, uint8_t* out, const uint64_t* out_off, int wrap, uint32_t M);
// the layout and the frames of a BGZF batch (deflate_bgzf.hip)
__global__ void zs_k_bgzf_local(const uint32_t* blk_base, zs_block* blocks, zs_stream* segs, const uint32_t* sstream,
                                zs_stream* streams, uint64_t* segx, uint64_t* tile, uint32_t M);
__global__ void zs_k_bgzf_place(const uint32_t* blk_base, zs_block* blocks, zs_stream* segs, const uint32_t* sfirst,
                                const uint32_t* sstream, zs_stream* streams, const uint64_t* segx, const uint64_t* tile,
                                const uint32_t* out_cap, uint8_t* out, const uint64_t* out_off, uint32_t M, uint32_t n);
__global__ void zs_k_bgzf_frame(const zs_stream* segs, const uint32_t* sstream, const zs_stream* streams,
                                const uint32_t* seg_len, const uint32_t* seg_check, uint8_t* out,
                                const uint64_t* out_off, uint32_t M, uint32_t n);
__global__ void zs_k_bgzf_stored(const uint8_t* in, const uint64_t* seg_in_off, const uint32_t* seg_len,
                                 const uint32_t* seg_check, const uint32_t* sfirst, const uint32_t* sstream,
                                 const uint32_t* in_len, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                 uint32_t B, uint32_t M, int32_t* status, uint32_t* out_len_res);
__global__ void zs_k_emit(const uint8_t* in, const uint64_t* in_off, const uint64_t* pos_base, const uint32_t* blk_base,
                          const uint32_t* syms, const zs_block* blocks, const zs_stream* streams, const uint32_t* codes,
                          const uint32_t* hdr, uint8_t* out, const uint64_t* out_off, int wrap);
__global__ void zs_k_stored(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                            const uint64_t* out_off, const uint32_t* out_cap, const uint32_t* check, int wrap,
                            int32_t* status, uint32_t* out_len_res);
__global__ void zs_k_wrap(const zs_stream* streams, uint8_t* out, const uint64_t* out_off, const uint32_t* in_len,
                          int wrap, int level, int nstreams, int strategy);
__global__ void zs_k_checksum(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t* check,
                              int kind, const uint32_t* seeds = nullptr);
// ... of long streams in parts of 1 << part_lg bytes (zs_plan_checksum): a wave per part, then a wave per stream
__global__ void zs_k_checksum_parts(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                    const uint32_t* pfirst, const uint32_t* pstream, uint32_t part_lg, uint32_t* vals,
                                    int kind);
__global__ void zs_k_checksum_fold(const uint32_t* in_len, const uint32_t* pfirst, uint32_t part_lg,
                                   const uint32_t* vals, uint32_t* check, int kind, const uint32_t* seeds);
__global__ void zs_k_selftest(uint32_t* bad, int rounds);
// a gzip file's members found from its bytes (inflate_members.hip): the candidates' scan, the
// members sized from offset 0 and from every candidate, the starts a bound stopped sized to the end, the
// per-stream join of the decoded members' results
template <bool EMIT>
__global__ void zs_k_members_scan(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* stile,
                                  uint32_t n, uint64_t* tcount, uint32_t* cand, uint64_t cap);
__global__ void zs_k_members_size(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* stile,
                                  uint32_t n, const uint64_t* tpre, const uint32_t* cand, uint64_t cap, uint32_t pass,
                                  zs_sync_rec* rec);
__global__ void zs_k_members_tail(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* tstream,
                                  const uint32_t* tstart, uint32_t m, zs_sync_rec* rec);
__global__ void zs_k_members_stitch(const uint32_t* rfirst, const uint32_t* soff, const uint32_t* opos,
                                    const int32_t* seg_status, const int32_t* seg_phase, const int32_t* seg_msg,
                                    const uint32_t* seg_len, const uint32_t* seg_used, uint32_t n, int32_t* status,
                                    int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed, uint32_t* cklen,
                                    const uint8_t* trusted);
// the same search over BGZF files (inflate_bgzf.hip): zs_k_members_size's arguments, lanes and
// records, a start whose header can be trusted sized from BSIZE and ISIZE; trusted: one byte per record
__global__ void zs_k_bgzf_size(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* stile,
                               uint32_t n, const uint64_t* tpre, const uint32_t* cand, uint64_t cap, uint32_t pass,
                               zs_sync_rec* rec, uint8_t* trusted);
// BGZF ranges by virtual offset (inflate_bgzf_range.hip): the streams' fields from the plan's
// verdicts and the members' results, then the members' clipped bytes from staging to their places
__global__ void zs_k_bgzf_range_end(const uint8_t* in, const uint64_t* sl_off, const uint32_t* sl_len, const uint32_t* rce,
                                    uint32_t n, uint32_t* end);
__global__ void zs_k_bgzf_range_stitch(const uint32_t* rfirst, const uint32_t* soff, const uint32_t* opos,
                                       const uint32_t* take, const uint32_t* verdict, const uint32_t* vcons,
                                       const int32_t* seg_status, const int32_t* seg_phase, const int32_t* seg_msg,
                                       const uint32_t* seg_used, uint32_t n, int32_t* status, int32_t* phase,
                                       int32_t* msg, uint32_t* out_len, uint32_t* consumed, uint32_t* cklen,
                                       const uint8_t* trusted);
__global__ void zs_k_bgzf_range_place(const uint8_t* stage, const uint64_t* stoff, const uint32_t* ocap,
                                      const uint32_t* seg_len, const uint32_t* skip, const uint32_t* take,
                                      const uint32_t* opos, const uint32_t* rstream, const uint32_t* out_len,
                                      const uint64_t* dst, const uint32_t* ptile, uint32_t M, uint8_t* out);
