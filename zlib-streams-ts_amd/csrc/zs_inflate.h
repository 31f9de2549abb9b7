// zs_inflate.h -- inflate kernel interface (inflate.hip) and message table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zs_plan.h"  // zs_inf_large, zs_inf_expands

#define ZS_PHASE_NONE_ 0
#define ZS_PHASE_PROCESS_ 2
#define ZS_PHASE_FINISH_ 3
// inflate kernel flags
#define ZS_INF_REF_WRAP 1  // reproduce the reference's inflate_fast window-wrap copy (inffast.ts:133-147)

// z_stream messages (inflate.ts:397-1031, inffast.ts:108,197,210)
enum zs_msg_id {
  ZS_MSG_NONE = 0,
  ZS_MSG_HEADER_CHECK,
  ZS_MSG_METHOD,
  ZS_MSG_WINDOW,
  ZS_MSG_FLAGS,
  ZS_MSG_HEADER_CRC,
  ZS_MSG_BLOCK_TYPE,
  ZS_MSG_STORED_LEN,
  ZS_MSG_TOO_MANY,
  ZS_MSG_TOO_MANY_D64,
  ZS_MSG_CODE_LENGTHS,
  ZS_MSG_REPEAT,
  ZS_MSG_MISSING_EOB,
  ZS_MSG_LITLEN_SET,
  ZS_MSG_DIST_SET,
  ZS_MSG_LITLEN_CODE,
  ZS_MSG_DIST_CODE,
  ZS_MSG_TOO_FAR,
  ZS_MSG_DATA_CHECK,
  ZS_MSG_LENGTH_CHECK,
  ZS_MSG_CAPACITY,
  ZS_MSG_RESTART,  // the restart entries: "restart points do not decode the stream"
  ZS_MSG_UNUSED_22,   // no message: the index behind the restart entries' stays empty (callers test it for "")
  ZS_MSG_BGZF_RANGE,  // the _bgzf_range entries: "virtual offsets do not follow a chain of BGZF blocks"
  ZS_MSG_COUNT
};

struct zs_inflate_result {
  int32_t status;
  int32_t phase;
  int32_t msg;
  uint32_t out_len;
  uint32_t consumed;
};

// Outcome of the lane-per-member fast path (inflate_lane.hip).
struct zs_lane_res {
  uint32_t bail;      // 0: decoded cleanly; 1: the exact path decides
  uint32_t out_len;
  uint32_t consumed;
  uint32_t want;      // trailer check value (zlib: adler32, gzip: crc32)
};

// Preset dictionaries of a batch (inflateSetDictionary, inflate.ts:1220-1249), all
// device memory: member s has the len[s] bytes at dict + off[s] (len[s] = 0: none;
// members may share one), whose adler32 is adler[id[s]] (zlib members: compared
// with the header's DICTID).  dict = nullptr: a batch without dictionaries.
struct zs_dict_args {
  const uint8_t* dict;
  const uint64_t* off;
  const uint32_t* len;
  const uint32_t* id;
  const uint32_t* adler;
};

__global__ void zs_k_inflate(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                             const uint64_t* out_off, const uint32_t* out_cap, int wbits, zs_inflate_result* res,
                             const zs_lane_res* only, int flags, zs_dict_args dd = {});
struct zs_lane_tabs;
// DICT: the instances of a batch with dictionaries (dd is read by them only)
template <int RT, bool REFW, bool DICT = false>
__global__ void zs_k_inflate_lane(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                  const uint64_t* out_off, const uint32_t* out_cap, int wbits, uint32_t n_members,
                                  zs_lane_tabs* tabs, zs_lane_res* res, uint32_t* lens_out, int flags,
                                  uint32_t wave_min, const uint32_t* list, zs_dict_args dd = {});
template <bool REFW>
__global__ void zs_k_inflate_wave(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                  const uint64_t* out_off, const uint32_t* out_cap, int wbits, const uint32_t* list,
                                  uint32_t n_list, zs_lane_res* res, uint32_t* lens_out, const uint32_t* n_dev);
__global__ void zs_k_inflate_lane_verify(zs_lane_res* res, const uint32_t* check, uint32_t n);
size_t zs_inflate_smem_bytes(int wbits);
size_t zs_inflate_lane_lds_bytes(bool root);
size_t zs_inflate_lane_scratch_bytes();
size_t zs_inflate_wave_lds_bytes(bool d64);

// a stream decoded from its restart points (inflate_restart.hip): the segments copied and
// closed, the staging route's copy back, the results joined per stream, the trailer's check
__global__ void zs_k_restart_gather(const uint8_t* in, const uint64_t* src, const uint32_t* slen, const uint32_t* glen,
                                    const uint64_t* goff, const uint32_t* gtile, uint32_t M, uint8_t* gather,
                                    uint32_t* mark);
__global__ void zs_k_restart_place(const uint8_t* stage, const uint64_t* stoff, const uint32_t* ocap,
                                   const uint32_t* seg_len, const uint64_t* dst, const uint32_t* ptile, uint32_t M,
                                   uint8_t* out);
__global__ void zs_k_restart_stitch(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                    const uint32_t* over, const uint32_t* rfirst, const uint32_t* soff,
                                    const uint32_t* slen, const uint32_t* olen, const uint32_t* opos, const uint32_t* mark,
                                    const int32_t* seg_status, const int32_t* seg_msg, const uint32_t* seg_len,
                                    const uint32_t* seg_used, int wbits, uint32_t n, int32_t* status, int32_t* phase,
                                    int32_t* msg, uint32_t* out_len, uint32_t* consumed, uint32_t* want);
__global__ void zs_k_restart_check(const uint32_t* sum, const uint32_t* want, int wbits, uint32_t n, int32_t* status,
                                   int32_t* phase, int32_t* msg, uint32_t* out_len, uint32_t* consumed, uint32_t* check);

// restart points found from the bytes (inflate_sync.hip): the first points, the candidates
// (<false> counts per tile, <true> emits), the count-only decode from every start
struct zs_sync_rec;
__global__ void zs_k_sync_first(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, int wbits, uint32_t n,
                                uint32_t* first);
template <bool EMIT>
__global__ void zs_k_sync_scan(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* first,
                               const uint32_t* stile, uint32_t n, uint64_t* tcount, uint32_t* cand, uint64_t cap);
__global__ void zs_k_sync_size(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* first,
                               const uint32_t* stile, uint32_t n, const uint64_t* tpre, const uint32_t* cand, uint64_t cap,
                               uint32_t pass, zs_sync_rec* rec);
__global__ void zs_k_sync_tail(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* tstream,
                               const uint32_t* tstart, uint32_t m, zs_sync_rec* rec);
