/*
 * zs_gpu.h -- C-ABI of the MI355X batched deflate/inflate engine
 * (libzsgpu.so, built from zlib-streams-ts_amd/csrc).
 *
 * The drop-in boundary for zlib-streams-ts's hot path.  Each batch entry runs
 * N independent streams, and stream i produces exactly the bytes (or the
 * error) that piping in[i] alone through the reference's web-streams layer
 * yields when the whole buffer is passed in ONE write() followed by close():
 *
 *   zs_deflate_batch*  replaces, per stream,
 *       new CompressionStream(format, {level})            src/mod/streams.ts:242-251
 *         -> createZeroCopyCompressionTransform           src/mod/streams.ts:216-228
 *         -> deflateInit2_(s, level, 8, wbits, 8, 0)      src/mod/deflate/deflate.ts:253-343
 *         -> deflate(s, Z_NO_FLUSH) per 32 KiB, deflate(s, Z_FINISH), deflateEnd
 *                                                         src/mod/deflate/deflate.ts:716-1013
 *   zs_inflate_batch*  replaces, per stream,
 *       new DecompressionStream(format)                   src/mod/streams.ts:253-262
 *         -> inflateInit2_(s, wbits) / inflate / inflateEnd
 *                                                         src/mod/inflate/inflate.ts:174-192,332-1185
 *   zs_crc32_batch / zs_adler32_batch replace           src/mod/common/crc32.ts:26-58,
 *                                                         src/mod/common/adler32.ts:4-25
 *
 * Conventions
 *   - Plain pointers and sizes only.  Buffers named d_* are device pointers
 *     (HBM) on the context's device; the per-stream layout arrays (offsets,
 *     lengths, capacities) are host arrays owned by the caller for the call.
 *   - wbits follows the format -> windowBits mapping of streams.ts:220,233:
 *     -15 "deflate-raw", 15 "deflate" (zlib), 31 "gzip", -16 "deflate64-raw"
 *     (inflate only).  level: 0..9 or -1 (= 6, deflate.ts:268-270).
 *   - Status codes are the reference's Z_* values (common/constants.ts:21-29).
 *     Per-stream status: ZS_STREAM_END on success; ZS_BUF_ERROR if out_cap[i]
 *     is too small (size outputs with zs_deflate_bound); decode errors as the
 *     reference reports them (see zs_inflate_batch_device).
 *   - Return value of every call: ZS_OK, or ZS_STREAM_ERROR for invalid
 *     arguments (the reference's deflateInit2_ validation, deflate.ts:281-294,
 *     which the stream layer reports as "init failed: -2", streams.ts:53), or
 *     ZS_MEM_ERROR when device memory cannot be obtained.  zs_last_error()
 *     describes the last failure on the calling thread.
 *   - Output offsets and capacities of the device entry points must be
 *     multiples of 4 bytes (the engine writes 32-bit words; ZS_STREAM_ERROR
 *     otherwise): no store leaves [out_off[i], out_off[i] + out_cap[i]).  Only
 *     the device entries have that rule.  BOTH host-buffer entries,
 *     zs_deflate_batch_ex and zs_inflate_batch_ex with their siblings, take
 *     exact, unaligned capacities and any output offset: they round the
 *     capacity up inside their own staging, report Z_BUF_ERROR past the
 *     caller's value (never for a capacity that is enough but no multiple of
 *     4) and copy back only the bytes produced.  Inputs may be packed at any
 *     byte offset.
 */
#ifndef ZS_GPU_H
#define ZS_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_OK 0
#define ZS_STREAM_END 1
#define ZS_NEED_DICT 2
#define ZS_STREAM_ERROR (-2)
#define ZS_DATA_ERROR (-3)
#define ZS_MEM_ERROR (-4)
#define ZS_BUF_ERROR (-5)

/* stream-layer phase of a per-stream failure (streams.ts:53,117,170) */
#define ZS_PHASE_NONE 0
#define ZS_PHASE_INIT 1
#define ZS_PHASE_PROCESS 2
#define ZS_PHASE_FINISH 3

typedef struct zs_ctx zs_ctx;

/* One context per device (one process per GPU).  Workspaces grow on demand
 * and are reused across calls; a context is not re-entrant across threads. */
int zs_ctx_create(int device, zs_ctx **out);
void zs_ctx_destroy(zs_ctx *ctx);
const char *zs_last_error(void);
const char *zs_version(void);

/* Re-checks the hardware property the fast chain builders use: same-address
 * LDS atomics of one wave instruction apply in lane order (gfx950).  Writes the
 * number of violations (0 expected).  zs_ctx_create runs it; when it does not
 * hold, the context uses the ballot-ranked builders instead (option lane_order
 * = 0, which can also be set by hand; the output bytes are the same).  No
 * reference counterpart (engine self-check). */
int zs_selftest(zs_ctx *ctx, uint64_t *violations);

/* deflateBound for a fresh stream with memLevel 8 (deflate.ts:615-674). */
uint64_t zs_deflate_bound(uint64_t source_len, int wbits);

/* Batched compression, device-resident buffers.  Enqueued on hip_stream (a
 * hipStream_t, or NULL for the context's own stream); returns once enqueued.
 * d_status[i] / d_out_len[i] (device int32 / uint32 arrays) are written. */
int zs_deflate_batch_device(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *d_in,
                            const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out, const uint64_t *out_off,
                            const uint32_t *out_cap, int32_t *d_status, uint32_t *d_out_len, void *hip_stream);

/* Same, host buffers: copies in, runs, copies out, synchronizes. */
int zs_deflate_batch(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                     const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                     int32_t *status, uint32_t *out_len);

/* Batched decompression, device-resident buffers.  Per stream: d_status[i]
 * (ZS_STREAM_END, or the Z_* code the stream layer reports), d_phase[i]
 * (ZS_PHASE_PROCESS / ZS_PHASE_FINISH for failures), d_msg[i] (index into
 * zs_inflate_message()), d_out_len[i], d_consumed[i] (input bytes used up to
 * the end of the stream; trailing bytes are ignored, streams.ts:74-76). */
int zs_inflate_batch_device(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *d_in, const uint64_t *in_off,
                            const uint32_t *in_len, uint8_t *d_out, const uint64_t *out_off, const uint32_t *out_cap,
                            int32_t *d_status, int32_t *d_phase, int32_t *d_msg, uint32_t *d_out_len,
                            uint32_t *d_consumed, void *hip_stream);

int zs_inflate_batch(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                     const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                     int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed);

/* The same batch entries with the per-stream check value: check[i] is the
 * reference's strm.adler after stream i (deflate.ts:155-159,462,778,788;
 * inflate.ts:105,1014,1080): the adler32 (zlib) / crc32 (gzip) of the stream's
 * uncompressed bytes; for deflate-raw compression 1 (adler32(0), never updated
 * without a wrapper), for raw / deflate64-raw decompression 0 (createStream's
 * initial value, common/utils.ts:49); 0 for a stream that failed.  d_check /
 * check may be NULL (then these are the calls above). */
int zs_deflate_batch_device_ex(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *d_in,
                               const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                               const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                               uint32_t *d_out_len, uint32_t *d_check, void *hip_stream);
int zs_deflate_batch_ex(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *in,
                        const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                        const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check);
int zs_inflate_batch_device_ex(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *d_in,
                               const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                               const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status, int32_t *d_phase,
                               int32_t *d_msg, uint32_t *d_out_len, uint32_t *d_consumed, uint32_t *d_check,
                               void *hip_stream);
int zs_inflate_batch_ex(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                        const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                        int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed,
                        uint32_t *check);

/* Unbounded decode, as DecompressionStream (streams.ts:46,132-182: pooled 64 KiB
 * output buffers until Z_STREAM_END, no output cap).  Host buffers; the outputs
 * land in ONE buffer the library allocates: on ZS_OK *out points to it, stream i
 * at (*out)[out_off[i]], out_len[i] bytes; release it with zs_free().  Members
 * are retried, alone, with eight times the room until they fit, so no member
 * reports the capacity message unless its output exceeds 4 GiB - 4 bytes (the
 * u32 length of this ABI). */
int zs_inflate_batch_auto(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, uint8_t **out, uint64_t *out_off, int32_t *status, int32_t *phase,
                          int32_t *msg, uint32_t *out_len, uint32_t *consumed, uint32_t *check);
void zs_free(void *p);

/* Multi-GPU pool (SURVEY.md 8(b) "device mask", 8(e)): one context per device
 * of device_mask (bit d = HIP device d; 0 = every visible device).  A batch is
 * partitioned into contiguous stream ranges [k n / G, (k + 1) n / G) over the G
 * devices, one host thread per device; each shard writes straight into the
 * caller's arrays (offsets are absolute), so results are identical to one
 * device's.  Same arguments and semantics as the single-context host calls.
 * One batch at a time per pool. */
typedef struct zs_pool zs_pool;
int zs_pool_create(uint64_t device_mask, zs_pool **out);
/* The same from a list of devices, in shard order; a device may appear more
 * than once (each entry gets its own context: the pool's sharding rehearsed on
 * one GPU).  ZS_STREAM_ERROR for a device that does not exist. */
int zs_pool_create_list(const int *devices, int n_devices, zs_pool **out);
void zs_pool_destroy(zs_pool *pool);
int zs_pool_size(const zs_pool *pool);
int zs_pool_device(const zs_pool *pool, int k);
int zs_pool_deflate_batch(zs_pool *pool, int level, int wbits, uint32_t n_streams, const uint8_t *in,
                          const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                          const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check);
int zs_pool_inflate_batch(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                          int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed,
                          uint32_t *check);
int zs_pool_inflate_batch_auto(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in,
                               const uint64_t *in_off, const uint32_t *in_len, uint8_t **out, uint64_t *out_off,
                               int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed,
                               uint32_t *check);

/* Decompression with preset dictionaries, raw deflate (-15) and zlib (15): each
 * stream is decoded as if the driver of the z_stream functions called
 * inflateSetDictionary(strm, dict, dict_len[i]) (inflate.ts:1220-1249) where
 * zlib's contract calls for it -- for raw deflate right after inflateInit2_, for
 * zlib when the first inflate() returns Z_NEED_DICT (FDICT set, inflate.ts:594-597),
 * after which inflate() is called again with the same buffers.  The window keeps a
 * dictionary's last 32,768 bytes (updatewindow, inflate.ts:282-324).
 *
 * The entries take the arguments of their counterparts above plus the
 * dictionaries: stream i has the dict_len[i] bytes at dict + dict_off[i]
 * (d_dict: device memory; dict: host memory).  dict_off / dict_len are host
 * arrays of n_streams entries; entries may alias, so the whole batch can share
 * one dictionary; a length of 0 means no dictionary; any byte offset is allowed.
 *  - zlib, FDICT set, adler32(dictionary) != DICTID: ZS_DATA_ERROR, phase
 *    ZS_PHASE_PROCESS, the empty message, no output (inflate.ts:1235-1241);
 *  - zlib, FDICT set, dict_len[i] == 0: ZS_NEED_DICT, as the entries above;
 *  - zlib, FDICT clear: inflateSetDictionary is never called, the dictionary is
 *    ignored;
 *  - a distance past dictionary plus output: "invalid distance too far back";
 *  - check[i] (strm.adler after the stream): zlib the adler32 of the output only
 *    (the check restarts after DICTID, inflate.ts:592), raw 0;
 *  - gzip (31: never in DICT mode, inflate.ts:1229) and deflate64-raw (-16) with
 *    any non-zero dict_len: the call returns ZS_STREAM_ERROR.
 * (updatewindow indexes its source from end.length rather than from its length
 * argument; this ABI passes (pointer, length), so dict.length == dictLength
 * always and that quirk of the reference is unreachable.)  A call whose
 * dict_len are all 0 is the counterpart's call. */
/* inflate.ts:1220-1249, :594-597 -- device buffers (as zs_inflate_batch_device_ex) */
int zs_inflate_batch_dict_device(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                 const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                 const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                 int32_t *d_phase, int32_t *d_msg, uint32_t *d_out_len, uint32_t *d_consumed,
                                 uint32_t *d_check, void *hip_stream, const uint8_t *d_dict,
                                 const uint64_t *dict_off, const uint32_t *dict_len);
/* inflate.ts:1220-1249, :594-597 -- host buffers (as zs_inflate_batch_ex) */
int zs_inflate_batch_dict(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                          int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed,
                          uint32_t *check, const uint8_t *dict, const uint64_t *dict_off, const uint32_t *dict_len);
/* inflate.ts:1220-1249, :594-597 -- unbounded output (as zs_inflate_batch_auto) */
int zs_inflate_batch_dict_auto(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                               const uint32_t *in_len, uint8_t **out, uint64_t *out_off, int32_t *status,
                               int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed, uint32_t *check,
                               const uint8_t *dict, const uint64_t *dict_off, const uint32_t *dict_len);
/* inflate.ts:1220-1249, :594-597 -- the pool (as zs_pool_inflate_batch) */
int zs_pool_inflate_batch_dict(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in,
                               const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                               const uint32_t *out_cap, int32_t *status, int32_t *phase, int32_t *msg,
                               uint32_t *out_len, uint32_t *consumed, uint32_t *check, const uint8_t *dict,
                               const uint64_t *dict_off, const uint32_t *dict_len);
/* inflate.ts:1220-1249, :594-597 -- the pool, unbounded output (as zs_pool_inflate_batch_auto) */
int zs_pool_inflate_batch_dict_auto(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in,
                                    const uint64_t *in_off, const uint32_t *in_len, uint8_t **out, uint64_t *out_off,
                                    int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len,
                                    uint32_t *consumed, uint32_t *check, const uint8_t *dict,
                                    const uint64_t *dict_off, const uint32_t *dict_len);

/* Compression against preset dictionaries, raw deflate (-15) and zlib (15): stream
 * i is the bytes of deflateInit2_(level, Z_DEFLATED, wbits, 8, Z_DEFAULT_STRATEGY),
 * then deflateSetDictionary(strm, dict, dict_len[i]) (deflate.ts:367-424) when
 * dict_len[i] > 0, then the stream layer's one write() + close() as in the
 * entries above.  The window takes a dictionary's last 32,768 bytes (deflate.ts:383-392).
 *
 * The entries take the arguments of their _ex counterparts plus the dictionaries,
 * with the conventions of the zs_inflate_batch_dict* entries: dict_off / dict_len
 * are host arrays of n_streams entries, entries may alias, a length of 0 means no
 * dictionary (that stream's bytes are the plain entries'), any byte offset.
 *  - zlib: FDICT is set, FCHECK taken with it, and DICTID -- the adler32 of ALL
 *    dict_len[i] bytes -- follows the header (deflate.ts:767-778); the trailer and
 *    check[i] are the adler32 of the data alone (the check restarts at 1);
 *  - raw: no header; check[i] stays 1;
 *  - gzip (31; deflateSetDictionary returns Z_STREAM_ERROR for wrap 2,
 *    deflate.ts:373) with any non-zero dict_len: the call returns ZS_STREAM_ERROR;
 *  - level 0 with any non-zero dict_len: the call returns ZS_STREAM_ERROR (not
 *    built: deflate_stored's block cuts after a dictionary depend on the stream
 *    layer's buffer sizes, which no available yardstick reproduces);
 *  - invalid level, short capacity (Z_BUF_ERROR), statuses and messages as the
 *    plain entries.  Size outputs with zs_deflate_bound_dict.
 * A call whose dict_len are all 0 is the counterpart's call. */
/* deflateBound after deflateSetDictionary (deflate.ts:633: four more bytes for
 * DICTID in a zlib stream): zs_deflate_bound, plus 4 for wbits 15 and dict_len > 0. */
uint64_t zs_deflate_bound_dict(uint64_t source_len, int wbits, uint64_t dict_len);
/* deflate.ts:367-424, :767-778 -- device buffers (as zs_deflate_batch_device_ex) */
int zs_deflate_batch_dict_device(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                 const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                 const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                 uint32_t *d_out_len, uint32_t *d_check, void *hip_stream, const uint8_t *d_dict,
                                 const uint64_t *dict_off, const uint32_t *dict_len);
/* deflate.ts:367-424, :767-778 -- host buffers (as zs_deflate_batch_ex) */
int zs_deflate_batch_dict(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *in,
                          const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                          const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check,
                          const uint8_t *dict, const uint64_t *dict_off, const uint32_t *dict_len);
/* deflate.ts:367-424, :767-778 -- the pool (as zs_pool_deflate_batch) */
int zs_pool_deflate_batch_dict(zs_pool *pool, int level, int wbits, uint32_t n_streams, const uint8_t *in,
                               const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                               const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check,
                               const uint8_t *dict, const uint64_t *dict_off, const uint32_t *dict_len);

/* Compression strategies: stream i is the bytes of deflateInit2_(level, Z_DEFLATED,
 * wbits, 8, strategy) and the stream layer's one write() + close(), for every strategy
 * the reference validates (deflate.ts:289-290) and dispatches on (deflate.ts:923-931). */
#define ZS_DEFAULT_STRATEGY 0 /* deflate.ts:923-931: the level's own deflate_fast / deflate_slow */
#define ZS_FILTERED 1         /* deflate.ts:1381-1387: deflate_slow drops a new match of at most 5 bytes */
#define ZS_HUFFMAN_ONLY 2     /* deflate.ts:1525-1565: deflate_huff, every byte a literal */
#define ZS_RLE 3              /* deflate.ts:1450-1523: deflate_rle (see option rle_ref) */
#define ZS_FIXED 4            /* trees.ts:567: no dynamic trees (stored blocks are still chosen, trees.ts:574) */
/* The entries take the arguments of zs_deflate_batch_device_ex / zs_deflate_batch_ex /
 * zs_pool_deflate_batch with `strategy` behind `level`.
 *  - strategy below 0 or above 4: the call returns ZS_STREAM_ERROR (deflate.ts:289-290,
 *    "init failed: -2");
 *  - ZS_DEFAULT_STRATEGY is the counterpart's call;
 *  - level 0 with any strategy is the plain level-0 path (deflate.ts:925 picks deflate_stored
 *    first; both wrappers already read "level < 2");
 *  - ZS_FILTERED at levels 1..3 is strategy 0's bytes (deflate_fast has no filtered branch);
 *  - ZS_HUFFMAN_ONLY and above clear the zlib header's level bits (deflate.ts:757) and set
 *    gzip's XFL to 4 below level 9 (deflate.ts:798);
 *  - ZS_RLE follows option rle_ref: 1 (default) the reference, whose scan compares the
 *    previous byte's value with the scan index (deflate.ts:1469-1481) and so never finds a
 *    run -- the bytes are ZS_HUFFMAN_ONLY's; 0 zlib's deflate_rle (matches at distance 1).
 *    The pool's contexts keep the default;
 *  - preset dictionaries are not built with a strategy: there are no _dict forms of these
 *    entries;
 *  - statuses, check values, Z_BUF_ERROR and zs_deflate_bound (deflateBound does not look
 *    at the strategy) as the plain entries. */
/* deflate.ts:289-290, :923-931 -- device buffers (as zs_deflate_batch_device_ex) */
int zs_deflate_batch_strategy_device(zs_ctx *ctx, int level, int strategy, int wbits, uint32_t n_streams,
                                     const uint8_t *d_in, const uint64_t *in_off, const uint32_t *in_len,
                                     uint8_t *d_out, const uint64_t *out_off, const uint32_t *out_cap,
                                     int32_t *d_status, uint32_t *d_out_len, uint32_t *d_check, void *hip_stream);
/* deflate.ts:289-290, :923-931 -- host buffers (as zs_deflate_batch_ex) */
int zs_deflate_batch_strategy(zs_ctx *ctx, int level, int strategy, int wbits, uint32_t n_streams, const uint8_t *in,
                              const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                              const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check);
/* deflate.ts:289-290, :923-931 -- the pool (as zs_pool_deflate_batch) */
int zs_pool_deflate_batch_strategy(zs_pool *pool, int level, int strategy, int wbits, uint32_t n_streams,
                                   const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                                   const uint64_t *out_off, const uint32_t *out_cap, int32_t *status,
                                   uint32_t *out_len, uint32_t *check);

/* windowBits and memLevel: stream i is the bytes of deflateInit2_(level, Z_DEFLATED, wbits,
 * mem_level, Z_DEFAULT_STRATEGY) (deflate.ts:253-343) and the stream layer's one write() +
 * close(), for the whole range of both arguments.  The window is w_size = 1 << windowBits
 * bytes (a decoder with that much window can inflate the stream), the hash has mem_level + 7
 * bits, and a block closes after (1 << (mem_level + 6)) - 1 symbols (deflate.ts:295-336).
 * The entries take the arguments of zs_deflate_batch_device_ex / zs_deflate_batch_ex /
 * zs_pool_deflate_batch with `mem_level` behind `wbits`.
 *  - wbits: -9..-15 raw deflate, 8..15 zlib, 25..31 gzip.  8 runs as 9 and writes CINFO 1
 *    (deflate.ts:295-297); the zlib header's CINFO is windowBits - 8 and FCHECK follows it
 *    (deflate.ts:754-770); the gzip header does not change;
 *  - -8, 24, any other wbits: the call returns ZS_STREAM_ERROR, zs_last_error() "invalid window
 *    bits"; mem_level outside 1..9: ZS_STREAM_ERROR, "invalid memLevel" (deflate.ts:281-294,
 *    "init failed: -2").  Both are checked before the context is looked at;
 *  - wbits -15, 15 or 31 with mem_level 8 is the counterpart's call: the same plan, kernels
 *    and bytes;
 *  - level 0 with any other parameters: ZS_STREAM_ERROR (not built: deflate_stored's cuts then
 *    depend on w_size, pending_buf_size and the stream layer's output buffers, which no
 *    available yardstick reproduces);
 *  - preset dictionaries and strategies are not built with these parameters: there are no
 *    _dict or _strategy forms of these entries;
 *  - statuses, check values, Z_BUF_ERROR and the 4-byte alignment rule of the device form as
 *    the plain entries.  Size outputs with zs_deflate_bound_params. */
/* deflateBound (deflate.ts:619-673) for deflateInit2_'s windowBits (as above) and mem_level: with
 * w_bits != 15 or hash_bits != 15 it is (w_bits <= hash_bits && level ? fixedlen : storelen) +
 * wraplen (deflate.ts:669-671), fixedlen = n + (n >> 3) + (n >> 8) + (n >> 9) + 4, storelen =
 * n + (n >> 5) + (n >> 7) + (n >> 11) + 7; otherwise zs_deflate_bound's formula.  0 for
 * parameters the entries refuse. */
uint64_t zs_deflate_bound_params(uint64_t source_len, int wbits, int mem_level, int level);
/* deflate.ts:253-343 -- device buffers (as zs_deflate_batch_device_ex) */
int zs_deflate_batch_params_device(zs_ctx *ctx, int level, int wbits, int mem_level, uint32_t n_streams,
                                   const uint8_t *d_in, const uint64_t *in_off, const uint32_t *in_len,
                                   uint8_t *d_out, const uint64_t *out_off, const uint32_t *out_cap,
                                   int32_t *d_status, uint32_t *d_out_len, uint32_t *d_check, void *hip_stream);
/* deflate.ts:253-343 -- host buffers (as zs_deflate_batch_ex) */
int zs_deflate_batch_params(zs_ctx *ctx, int level, int wbits, int mem_level, uint32_t n_streams, const uint8_t *in,
                            const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                            const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check);
/* deflate.ts:253-343 -- the pool (as zs_pool_deflate_batch) */
int zs_pool_deflate_batch_params(zs_pool *pool, int level, int wbits, int mem_level, uint32_t n_streams,
                                 const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                                 const uint64_t *out_off, const uint32_t *out_cap, int32_t *status,
                                 uint32_t *out_len, uint32_t *check);

/* Z_FULL_FLUSH points: one stream's pieces compressed in parallel.  Stream i has the flush
 * positions 0 <= p_1 < p_2 < ... < p_k <= in_len[i], all given with the call, and its output is
 * what the z_stream functions produce for deflateInit2_(level, Z_DEFLATED, wbits, 8,
 * Z_DEFAULT_STRATEGY); then for each piece in[p_(j-1) .. p_j) the stream layer's 32 KiB
 * sub-chunks with Z_NO_FLUSH and deflate(Z_FULL_FLUSH) until it has drained; then the rest and
 * Z_FINISH (deflate.ts:716-989).  At a full flush the reference closes the pending block if it
 * holds symbols (deflate.ts:1343,1441), writes an empty stored block -- 00 00 FF FF behind three
 * header bits and the padding to a byte -- clears the hash and, all input consumed, sets strstart
 * = block_start = insert = 0 (deflate.ts:923-961, the branch at 942-955): the bytes behind a
 * point are those of a fresh stream over the next piece, they start on a byte boundary, and a
 * decoder can restart there (pigz -i, seekable .gz).  The pieces are independent, so one long
 * stream with flush points uses the whole device as a batch of as many streams does.
 * This stays a one-shot batch: the whole input and every position are given in one call.
 * The entries take the arguments of zs_deflate_batch_device_ex / zs_deflate_batch_ex /
 * zs_pool_deflate_batch, then `flush` and the positions: flush_first is a host array of
 * n_streams + 1 entries and stream i's positions are flush_pos[flush_first[i] ..
 * flush_first[i + 1]) (host array, increasing).
 *  - flush must be ZS_FULL_FLUSH.  Z_PARTIAL_FLUSH (1), Z_SYNC_FLUSH (2) and Z_BLOCK (5):
 *    ZS_STREAM_ERROR, "flush mode not built"; anything else: ZS_STREAM_ERROR, "invalid flush"
 *    (deflate.ts:720).  Checked before the context is looked at;
 *  - a null flush_first, or a null flush_pos with any position: ZS_STREAM_ERROR, "null flush arrays";
 *  - equal or decreasing positions, or one past in_len[i]: ZS_STREAM_ERROR, "invalid flush
 *    positions" (a second flush with no input between is Z_BUF_ERROR in the reference,
 *    deflate.ts:742-743; no caller wants that, so the call is refused);
 *  - level 0 with any flush point: ZS_STREAM_ERROR (not built: deflate_stored's cuts depend on
 *    the stream layer's output buffers, as for dictionaries);
 *  - streams + flush points above 65,535 in one call: ZS_STREAM_ERROR (split the batch);
 *  - a flush at 0 writes the five marker bytes alone behind the wrapper's header; a flush at
 *    in_len[i] writes the marker and Z_FINISH then the empty final block 03 00; only the block
 *    Z_FINISH closes carries BFINAL;
 *  - the wrapper and check[i] cover the whole stream: adler32 / crc32 of all its bytes, the whole
 *    length in gzip's ISIZE;
 *  - a call whose streams have no flush point is the counterpart's call: the same plan, kernels
 *    and bytes;
 *  - preset dictionaries, strategies and windowBits / memLevel are not built with flush points:
 *    there are no _dict, _strategy or _params forms of these entries;
 *  - statuses, Z_BUF_ERROR (against the stream's out_cap[i]) and the 4-byte alignment rule of the
 *    device form as the plain entries.  Size outputs with zs_deflate_bound_flush. */
#define ZS_FULL_FLUSH 3 /* Z_FULL_FLUSH, common/constants.ts */
/* zs_deflate_bound + 12 n_flush: every extra piece costs at most the raw bound's constant 7 and
 * the marker's 5 bytes; the bound's shifted terms are sub-additive.  It bounds a primed call's output
 * too (n_flush points): a raw piece with a dictionary adds no bytes and its marker is the same 5. */
uint64_t zs_deflate_bound_flush(uint64_t source_len, int wbits, uint64_t n_flush);
/* deflate.ts:923-961 -- device buffers (as zs_deflate_batch_device_ex) */
int zs_deflate_batch_flush_device(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                  const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                  const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                  uint32_t *d_out_len, uint32_t *d_check, void *hip_stream, int flush,
                                  const uint64_t *flush_first, const uint32_t *flush_pos);
/* deflate.ts:923-961 -- host buffers (as zs_deflate_batch_ex) */
int zs_deflate_batch_flush(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *in,
                           const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                           const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check, int flush,
                           const uint64_t *flush_first, const uint32_t *flush_pos);
/* deflate.ts:923-961 -- the pool (as zs_pool_deflate_batch; sharded by stream) */
int zs_pool_deflate_batch_flush(zs_pool *pool, int level, int wbits, uint32_t n_streams, const uint8_t *in,
                                const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                                const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check,
                                int flush, const uint64_t *flush_first, const uint32_t *flush_pos);

/* Primed pieces: one stream's pieces compressed in parallel without the flush points' ratio loss
 * (pigz's construction).  Stream i has the positions 0 <= p_1 < ... < p_k <= in_len[i] of the _flush
 * entries, same arrays, same validation.  Its output is the stream's ordinary wrapper header (zlib: two
 * bytes, no FDICT; gzip: the ten-byte header, OS 255; raw: none); then for every piece d = in[a, b) in
 * order the bytes zlib 1.2.11 writes for deflateInit2_(level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY),
 * deflateSetDictionary(in[max(0, a - 32768), a)) if a > 0, the piece in the stream layer's 32 KiB
 * sub-chunks, and deflate(Z_SYNC_FLUSH) until drained -- deflate(Z_FINISH) for the last piece; then the
 * trailer over the whole input.  Every piece but the last ends on a byte boundary with BFINAL clear and
 * the marker 00 00 FF FF, and a distance into a piece's prime is a distance into the stream's earlier
 * output: the concatenation is ONE ordinary deflate stream that any decoder reads, at nearly the
 * single-stream ratio (a piece looks back across its point).  The first piece has no prime.
 *  - the piece rules are the flushed pieces': the pending block is closed only if it holds symbols, an
 *    empty last block is dropped, only the block Z_FINISH closes carries BFINAL;
 *  - all three formats are taken, gzip too (unlike the _dict entries): the pieces are raw, the wrapper
 *    is the stream's, check[i] is adler32 / crc32 of all its bytes and gzip's ISIZE the whole length;
 *  - refusals, statuses and messages as the _flush entries, less those of `flush`: null arrays, invalid
 *    positions, level 0 with a point, streams + points above 65,535 in one call, windowBits, level,
 *    and the device form's 4-byte alignment rule;
 *  - a call whose streams have no point is the _ex call: the same plan, kernels and bytes;
 *  - zs_last_flush_index returns the offsets behind the markers, as after a _flush call.  They are
 *    not restart points for a parallel decode: the bytes behind one refer back across it;
 *  - size outputs with zs_deflate_bound_flush: a raw piece with a dictionary adds no bytes (no FDICT,
 *    no DICTID) and the marker is the same five bytes;
 *  - the workspace grows with the sum of (prime + piece) over the pieces, not of the pieces alone;
 *  - caller dictionaries, strategies and windowBits / memLevel are not built with primed pieces. */
/* device buffers (as zs_deflate_batch_flush_device, without `flush`) */
int zs_deflate_batch_primed_device(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                   const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                   const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                   uint32_t *d_out_len, uint32_t *d_check, void *hip_stream,
                                   const uint64_t *flush_first, const uint32_t *flush_pos);
/* host buffers (as zs_deflate_batch_flush) */
int zs_deflate_batch_primed(zs_ctx *ctx, int level, int wbits, uint32_t n_streams, const uint8_t *in,
                            const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                            const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check,
                            const uint64_t *flush_first, const uint32_t *flush_pos);
/* the pool (as zs_pool_deflate_batch_flush; sharded by stream) */
int zs_pool_deflate_batch_primed(zs_pool *pool, int level, int wbits, uint32_t n_streams, const uint8_t *in,
                                 const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                                 const uint32_t *out_cap, int32_t *status, uint32_t *out_len, uint32_t *check,
                                 const uint64_t *flush_first, const uint32_t *flush_pos);

/* BGZF: one file's 64 KiB blocks compressed in parallel (SAM specification 4.1, "The BGZF compression
 * format").  Stream i of L = in_len[i] bytes with block size B becomes ceil(L / B) data blocks and then
 * the end-of-file block; an empty stream is the end-of-file block alone.  Data block j covers
 * in[jB .. min((j + 1)B, L)) and is one gzip member:
 *  - header, 18 bytes: 1f 8b 08 04 | 00 00 00 00 | 00 | ff | 06 00 | 42 43 02 00 | BSIZE -- FLG 4
 *    (FEXTRA), MTIME 0, XFL 0 at every level, OS 255, XLEN 6, the subfield 'B' 'C' with SLEN 2, and
 *    BSIZE = the block's total size - 1, little-endian u16 (htslib's bgzf_compress header; the plain
 *    gzip wrapper's XFL by level does not apply);
 *  - data, levels 1..9 (-1 is 6): the bytes zs_deflate_batch_ex(level, -15) produces for that piece
 *    alone -- deflateInit2_(level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY), all input, Z_FINISH.  Every
 *    piece is finished: its last block carries BFINAL and is padded to a byte, a piece whose symbols end
 *    on the 16,383-symbol cut keeps its trailing empty static block, and no marker is written;
 *  - data, level 0: one final stored block, 01 | LEN | ~LEN | the piece (RFC 1951 3.2.4).  These bytes
 *    are the definition; deflate_stored's cuts and the stream layer play no part;
 *  - trailer, 8 bytes: crc32 of the piece and the piece's length, little-endian u32 each.
 * The end-of-file block is the 28 bytes 1f8b08040000000000ff0600424302001b0003000000000000000000.
 * block_bytes is B: 0 means ZS_BGZF_BLOCK (65,280, htslib's BGZF_BLOCK_SIZE), 1 .. 65,280 are taken.
 * zs_deflate_bound(65280, -15) + 26 = 65,331 <= 65,536, so a block always fits BSIZE and no piece is
 * ever retried with less input; a block that came out larger all the same would fail its stream with
 * ZS_STREAM_ERROR, never write a wrapped BSIZE.
 * As a consequence the output is what bgzip built against zlib 1.2.11 writes single-threaded at the same
 * level (one-shot Z_FINISH and the 32 KiB feeding of the plain entry give the same bytes for a piece
 * this short); the contract is the bytes above.  bgzip, samtools, tabix, gzip -d and
 * zs_inflate_batch_bgzf* read it.
 * The entries take the arguments of zs_deflate_batch_device_ex / zs_deflate_batch_ex /
 * zs_pool_deflate_batch without wbits, then block_bytes.
 *  - status[i] and out_len[i] as the plain entries; ZS_BUF_ERROR against the stream's own out_cap[i],
 *    exactly, with nothing stored for that stream; check[i] is the crc32 of the WHOLE input (what a
 *    reader that concatenates the members computes), 0 for a failed stream; the device form's 4-byte
 *    alignment rule as the other device entries;
 *  - refused with ZS_STREAM_ERROR before the context is looked at, in this order: a level outside
 *    -1 .. 9 ("invalid level"); block_bytes above 65,280 ("invalid BGZF block size"); n_streams > 0 with
 *    a null offset, length or capacity array ("null arrays"); for the device entry streams + data
 *    blocks above 65,535 in the call ("too many BGZF blocks (streams + blocks above 65,535 in one
 *    call)": split the batch) -- a host call is checked chunk by chunk;
 *  - a call whose streams are all empty is still a BGZF call: end-of-file blocks;
 *  - preset dictionaries, strategies and windowBits / memLevel are not built: there are no _dict,
 *    _strategy or _params forms.  Size outputs with zs_deflate_bound_bgzf. */
#define ZS_BGZF_BLOCK 65280
/* The sum over the blocks of zs_deflate_bound(piece, -15) + 26, plus 28, in closed form; level 0's stored
 * form (piece + 5 + 26) is smaller, so one bound serves all levels.  0 for a block_bytes above 65,280. */
uint64_t zs_deflate_bound_bgzf(uint64_t source_len, uint32_t block_bytes);
/* device buffers (as zs_deflate_batch_device_ex) */
int zs_deflate_batch_bgzf_device(zs_ctx *ctx, int level, uint32_t n_streams, const uint8_t *d_in,
                                 const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                 const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                 uint32_t *d_out_len, uint32_t *d_check, void *hip_stream, uint32_t block_bytes);
/* host buffers (as zs_deflate_batch_ex) */
int zs_deflate_batch_bgzf(zs_ctx *ctx, int level, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                          int32_t *status, uint32_t *out_len, uint32_t *check, uint32_t block_bytes);
/* the pool (as zs_pool_deflate_batch; sharded by stream) */
int zs_pool_deflate_batch_bgzf(zs_pool *pool, int level, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                               const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                               int32_t *status, uint32_t *out_len, uint32_t *check, uint32_t block_bytes);
/* The blocks of the last BGZF compress call on the context, in the layout of zs_last_members: block_first
 * (n_streams + 1 entries, from 0), then at most `cap` blocks' block_in (the offset of the block's first
 * input byte) and block_out (the offset of the block's first byte in the stream's output).  Stream i has
 * its data blocks' entries and the end-of-file block's, (in_len[i], out_len[i] - 28): a .gzi index plus
 * the end; writing a .gzi file is the caller's job.  Returns the number of entries (0 when the last
 * compress call on the context was no BGZF call); waits for the call's kernels.  Right after a host
 * call that ran as several chunks too. */
uint64_t zs_last_bgzf_blocks(zs_ctx *ctx, uint64_t *block_first, uint32_t *block_in, uint32_t *block_out,
                             uint64_t cap);

/* Restart points: one stream's segments decoded in parallel.  Behind a Z_FULL_FLUSH marker (00 00 FF FF)
 * the bit stream is byte-aligned and the window empty; inflateSync (inflate.ts:1285-1337; syncsearch
 * :1267-1283) looks for those bytes and resets the stream there, the window with it.  These entries are
 * the decoder that zs_deflate_batch_flush* promises: stream i is given with its k_i >= 1 POINTS
 * (in_pos, out_pos), increasing in both coordinates; its k_i segments decode as independent members of
 * one batch -- so one long flushed stream uses the whole device -- and are joined, checked and reported
 * as one stream.
 *  - The first point is the start of the deflate data: in_pos the length of the wrapper's header
 *    (zs_wrapper_header_len: 0 raw, 2 zlib, gzip 10 plus FEXTRA / FNAME / FCOMMENT / FHCRC), out_pos 0.
 *    Every further point is a restart point: in_pos the offset in the stream's input of the first byte
 *    behind a marker, out_pos the uncompressed bytes before it.  Segment j is the input from point j to
 *    point j + 1, the last one to in_len[i], the trailer included.
 *  - The entries take the arguments of zs_inflate_batch_device_ex / zs_inflate_batch_ex /
 *    zs_pool_inflate_batch, then the points: restart_first is a host array of n_streams + 1 entries and
 *    stream i's points are (restart_in[k], restart_out[k]) for k in restart_first[i] ..
 *    restart_first[i + 1] (host arrays, the layout of flush_first / flush_pos).
 *  - ZS_STREAM_END when every segment decodes cleanly; every segment but the last has 00 00 FF FF in
 *    its last four bytes, consumes exactly its bytes and produces exactly the bytes up to the next
 *    point; the last ends at its own final block; the first point lies behind a well-formed header (zlib:
 *    method 8, CINFO <= 7, the check mod 31, no FDICT; gzip: magic, method 8, no reserved flag -- FHCRC
 *    is skipped, not verified); and the trailer agrees with the whole output (zlib: adler32, big-endian;
 *    gzip: crc32 and ISIZE, little-endian).  Then the output is what zlib's inflate produces for the whole
 *    stream, out_len[i] its length, consumed[i] reaches the end of the trailer (bytes behind it are
 *    ignored) and check[i] is as in zs_inflate_batch_ex.
 *  - zlib semantics, always: the segments decode with the instances that option inflate_ref_wrap = 0
 *    selects, whatever the context's option says (it is neither read nor changed).  The reference's
 *    window-wrap copy (inffast.ts:133-147) depends on its stream layer's inflate() call boundaries over
 *    the whole stream, and that layer never calls inflateSync: behind a reset there is no reference
 *    behaviour to reproduce.
 *  - Anything else: ZS_DATA_ERROR, ZS_PHASE_PROCESS, the message "restart points do not decode the
 *    stream", out_len = consumed = check = 0 -- except a stream whose output does not fit out_cap[i] (the
 *    last segment runs past it, or the last out_pos lies past it), which reports the plain entry's
 *    capacity outcome (ZS_BUF_ERROR, "output capacity exceeded").  The library does not fall back to a
 *    sequential decode: a caller who wants the reference's exact status for a broken stream runs the plain
 *    entry on it.  One failed stream does not touch the others; the bytes in its region are unspecified,
 *    but no store leaves [out_off[i], out_off[i] + out_cap[i]) rounded up to 4.
 *  - A raw stream has no trailer: a false point is caught by the marker bytes, the exact consumption and
 *    the exact length only.
 *  - A stream with only its first point is the plain decode of that stream with inflate_ref_wrap = 0.
 *  - Refused with ZS_STREAM_ERROR and a zs_last_error text, before the context is looked at: wbits -16
 *    (deflate64 has no flush on this side) or one the plain entry refuses; null point arrays; a stream
 *    without its first point; more than 67,108,863 segments in one call (every decoder runs a 64-thread
 *    workgroup per member, and a launch takes fewer than 2^32 threads); a first out_pos other than 0;
 *    an in_pos less than 5 bytes (a marker alone) behind the point before; a decreasing out_pos; an
 *    in_pos past in_len[i]; for the device entry, out_off / out_cap that are no multiples of 4.
 *  - Preset dictionaries and the unbounded (_auto) output are not built with restart points: there are
 *    no _dict or _auto forms.  A caller without an index uses the _sync entries below, which find the points.
 *  - Timing phases: "restart_gather", "restart_place", "restart_stitch", around the decoders' own. */
/* inflate.ts:1267-1337 -- device buffers (as zs_inflate_batch_device_ex) */
int zs_inflate_batch_restart_device(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                    const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                    const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                    int32_t *d_phase, int32_t *d_msg, uint32_t *d_out_len, uint32_t *d_consumed,
                                    uint32_t *d_check, void *hip_stream, const uint64_t *restart_first,
                                    const uint32_t *restart_in, const uint32_t *restart_out);
/* inflate.ts:1267-1337 -- host buffers (as zs_inflate_batch_ex) */
int zs_inflate_batch_restart(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                             const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                             int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed,
                             uint32_t *check, const uint64_t *restart_first, const uint32_t *restart_in,
                             const uint32_t *restart_out);
/* inflate.ts:1267-1337 -- the pool (as zs_pool_inflate_batch; sharded by stream) */
int zs_pool_inflate_batch_restart(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in,
                                  const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                                  const uint64_t *out_off, const uint32_t *out_cap, int32_t *status, int32_t *phase,
                                  int32_t *msg, uint32_t *out_len, uint32_t *consumed, uint32_t *check,
                                  const uint64_t *restart_first, const uint32_t *restart_in,
                                  const uint32_t *restart_out);
/* The length of the wrapper's header in front of the deflate data (inflate.ts:560-728): 0 for raw, 2 for
 * zlib; for gzip the parsed length -- 10, plus FEXTRA, FNAME, FCOMMENT and FHCRC where the flags name
 * them -- or 0 when the header is malformed (magic, method, a reserved flag) or does not end inside
 * in_len.  The first point of a stream.  Host arithmetic, no context. */
uint32_t zs_wrapper_header_len(int wbits, const uint8_t *in, uint32_t in_len);
/* The producer of an index: for the last zs_deflate_batch_flush_device / zs_deflate_batch_flush call on
 * the context, in the order of flush_pos, the offset within each stream's output (the wrapper's header
 * included) of the byte behind each marker -- the in_pos of a restart point whose out_pos is the flush
 * position.  Writes at most cap values, returns the count of flush points and synchronises the device.
 * 0 when the last compress call had no flush point.  Not offered on the pool (its shards' contexts are
 * its own). */
uint64_t zs_last_flush_index(zs_ctx *ctx, uint32_t *in_pos, uint64_t cap);

/* Restart points found from the bytes: a batched syncsearch (inflate.ts:1267-1283) for a caller who has
 * no index -- a seekable .gz of another writer, or this engine's own flushed output after the index was
 * lost.  The entries take EXACTLY the arguments of zs_inflate_batch_device_ex / zs_inflate_batch_ex /
 * zs_pool_inflate_batch (sharded by stream), no point arrays; for every stream they find the points and
 * run the restart entries' decode with them, whose contract holds with the found points:
 *  - For every stream that zlib's inflate decodes (the plain entry with inflate_ref_wrap = 0) the output,
 *    out_len, consumed and check are the plain entry's, with ZS_STREAM_END.  A stream without a marker is
 *    one segment and decodes as the plain entry does.  A stream that does not decode reports the restart
 *    entries' one failure (ZS_DATA_ERROR, ZS_PHASE_PROCESS, "restart points do not decode the stream",
 *    lengths 0) or their capacity outcome (ZS_BUF_ERROR, "output capacity exceeded"); its neighbours are
 *    untouched and no store leaves a stream's region rounded up to 4.  A malformed header is that failure
 *    too (a zlib stream with FDICT fails its header check).
 *  - How: a scan lists every offset behind the bytes 00 00 FF FF (CANDIDATES: a stored block may hold the
 *    same bytes); a count-only decode, one lane per START (the first point, behind the wrapper's header,
 *    and every candidate), records where and how the lane ended -- at the next candidate with a block
 *    just closed on a byte boundary, at the final block, at an error, or at its work bound -- the bytes
 *    it produced and how far its copies reach back before its start; the host follows the records from
 *    the first point, which gives the true points and their out_pos, and drops the points behind which
 *    the window is not empty (Z_SYNC_FLUSH / Z_PARTIAL_FLUSH markers: a stream with only those decodes
 *    as one segment, correct and no faster).  Where the chain stops before the final block (an error, or
 *    the work bound) the rest of the stream is one last segment.
 *  - The work bound: a lane started at candidate j of its stream stops at candidate j + sync_pass + 1
 *    (option "sync_pass", 1 .. 64, default 8), so every input byte is decoded by at most sync_pass + 1
 *    lanes whatever the bytes are.  A true segment that holds more than sync_pass false candidates ends
 *    the chain there: the decode stays correct and loses the points behind it (the rest of such a stream is
 *    sized once more, to its end, for how far its copies reach back: one more lane per such stream).
 *  - zlib semantics always, capacities must be given; wbits -16, one the plain entry refuses, a null
 *    out_cap and, for the device entry, out_off / out_cap that are no multiples of 4 are refused with
 *    ZS_STREAM_ERROR before the context is looked at, in that order.  More than 67,108,863 candidates plus
 *    streams in one call is ZS_STREAM_ERROR (the restart entries' segment cap): split the batch.
 *  - The points are planned on the host: the DEVICE entry synchronises hip_stream once in the middle
 *    (behind the scan and the size decode; a second time in a call whose candidates outgrow the list the
 *    context keeps from earlier calls, or in which a chain ends at its work bound), and is asynchronous
 *    from there on.  Its first points are computed
 *    on the device by the parse of zs_wrapper_header_len; the host entries run that function on their bytes.
 *  - The HOST entries run as one chunk (zs_last_host_chunks = 1) whatever the batch's size: the scan is
 *    not chunked.
 *  - Timing phases: "sync_scan", "sync_size", in front of the restart phases.
 *  - Not built: the chunked host pipeline for these calls; decoding only a range of segments (a seek);
 *    _auto capacities; dictionaries; deflate64; cutting at dynamic-block boundaries (what the split decode
 *    does inside one member); zs_last_restart_points on the pool.  These entries decode a gzip stream's
 *    first member, as the plain ones: multi-member gzip files are the _members entries' (below). */
int zs_inflate_batch_sync_device(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                 const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                 const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                 int32_t *d_phase, int32_t *d_msg, uint32_t *d_out_len, uint32_t *d_consumed,
                                 uint32_t *d_check, void *hip_stream);
int zs_inflate_batch_sync(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                          int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed,
                          uint32_t *check);
int zs_pool_inflate_batch_sync(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in,
                               const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                               const uint32_t *out_cap, int32_t *status, int32_t *phase, int32_t *msg,
                               uint32_t *out_len, uint32_t *consumed, uint32_t *check);
/* The points the last zs_inflate_batch_sync_device / zs_inflate_batch_sync call on the context used, in
 * the layout the restart entries take, every stream's first point included: restart_first gets
 * n_streams + 1 entries (from 0), restart_in / restart_out at most cap points; returns the count of
 * points.  A caller can keep them as an index and call zs_inflate_batch_restart* next time.  0 when the
 * last inflate call on the context was no _sync call.  Not offered on the pool. */
uint64_t zs_last_restart_points(zs_ctx *ctx, uint64_t *restart_first, uint32_t *restart_in, uint32_t *restart_out,
                                uint64_t cap);

/* Multi-member gzip files: BGZF / bgzip, WARC records, `cat a.gz b.gz`, appended logs.  The plain entries
 * decode a stream's first member and ignore the rest, as the reference does (streams.ts:74-76); these
 * decode EVERY member and concatenate the outputs, as gzip -d, zlib's gzread and Python's gzip.decompress
 * do.  gzip only.  The entries take EXACTLY the arguments of zs_inflate_batch_device_ex /
 * zs_inflate_batch_ex / zs_pool_inflate_batch (sharded by stream: members stay inside their stream).
 *  - The members of stream i, its bytes s[0..n): a member starts at 0; another starts at every position p
 *    directly behind a member's 8-byte trailer with p + 4 <= n, s[p..p+3) == 1f 8b 08 and
 *    (s[p+3] & 0xe0) == 0.  Where that test fails the stream ends and the bytes from p on are ignored (zero
 *    padding, garbage, a lone 1f 8b), as the plain entries ignore trailing bytes: consumed[i] = p.  Where
 *    it holds the bytes ARE a member, whatever follows: one that is truncated or corrupt fails the stream
 *    (zlib's gz_look, gzip -d).
 *  - Success: the output is the concatenation of the members' outputs, out_len[i] the total, status[i]
 *    ZS_STREAM_END, check[i] the crc32 of the whole output (= zs_crc32_combine over the members' values);
 *    every member's own CRC32 and ISIZE are verified.
 *  - Members decode with zlib semantics (the instances inflate_ref_wrap = 0 selects; the context's option
 *    is neither read nor changed, as in the restart entries): behind the first member there is no
 *    reference behaviour to reproduce.
 *  - Failure: let k be the first member that does not end with ZS_STREAM_END.  status[i], phase[i] and
 *    msg[i] are what zs_inflate_batch_ex with inflate_ref_wrap = 0 reports for the bytes s[start_k..n)
 *    alone; out_len[i] = out_pos_k (the complete members before k are in the region and valid);
 *    consumed[i] = start_k; check[i] = 0.  A total that does not fit out_cap[i] is this case: the first
 *    member that does not fit entirely is given no room and reports the plain entry's capacity outcome
 *    (ZS_BUF_ERROR, "output capacity exceeded"); so is a total above 2^32 - 1.  One failed stream does not
 *    touch the others; no store leaves [out_off[i], out_off[i] + out_cap[i]) rounded up to 4.
 *  - Refused with ZS_STREAM_ERROR before the context is looked at, in this order: wbits other than 31
 *    ("members are a gzip notion"), a null out_cap, for the device entry out_off / out_cap that are no
 *    multiples of 4.  More than 67,108,863 candidates plus streams in one call is ZS_STREAM_ERROR (the
 *    restart entries' segment cap): split the batch.
 *  - How: where member k + 1 starts is known once member k is decoded, so every plausible start is tried at
 *    once.  A scan lists every offset q >= 1 that passes the four-byte test (CANDIDATES: compressed data
 *    and stored blocks hold the same bytes); one lane per START (offset 0 and every candidate) parses the
 *    header, runs the _sync entries' count-only decode to the final block and requires the trailer's 8
 *    bytes; the host follows the records from 0.  The members then decode as the members of ONE gzip batch
 *    on the caller's own input (nothing is copied), in place when every out_pos is a multiple of 4, else
 *    through 4-aligned staging, and are joined per stream.
 *  - The work bound is the _sync entries': a lane started at candidate j of its stream reads no byte at or
 *    past candidate j + sync_pass + 1 (the same option), so every byte is decoded by at most sync_pass + 1
 *    bounded lanes.  A true member that holds more than sync_pass false candidates (a .tar.gz whose
 *    stored blocks hold .gz files) is sized once more by an unbounded lane, in a tail round: each round
 *    settles at least one member of each such stream.
 *  - The DEVICE entry synchronises hip_stream once in the middle (behind the scan and the size decode; a
 *    second time in a call whose candidates outgrow the list the context keeps) and once more per tail
 *    round, and is asynchronous from there on.  The HOST entries run as one chunk (zs_last_host_chunks = 1).
 *  - Timing phases: "members_scan", "members_size" and "members_stitch", around the decoders' own.
 *  - These entries recompute every length from the data.  The header-only fast path for BGZF (following BSIZE,
 *    trusting ISIZE for the positions) is the _bgzf entries' (below).
 *  - Not built: restart points inside members; _auto capacities; the chunked host pipeline; zlib or raw "members";
 *    decoding a range of members (a seek) of a plain multi-member file -- BGZF blocks between two virtual
 *    offsets are the _bgzf_range entries'; zs_last_members on the pool. */
int zs_inflate_batch_members_device(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                    const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                    const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                    int32_t *d_phase, int32_t *d_msg, uint32_t *d_out_len, uint32_t *d_consumed,
                                    uint32_t *d_check, void *hip_stream);
int zs_inflate_batch_members(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                             const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                             int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed,
                             uint32_t *check);
int zs_pool_inflate_batch_members(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in,
                                  const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                                  const uint32_t *out_cap, int32_t *status, int32_t *phase, int32_t *msg,
                                  uint32_t *out_len, uint32_t *consumed, uint32_t *check);
/* The members the last zs_inflate_batch_members_device / zs_inflate_batch_members call (or _bgzf call,
 * below) on the context decoded, in the layout of zs_last_restart_points: member_first gets n_streams + 1
 * entries (from 0), member_in / member_out at most cap members' (in_pos, out_pos), member 0 of a stream
 * being (0, 0); returns the count of members.  0 when the last inflate call on the context was neither.
 * Not offered on the pool. */
uint64_t zs_last_members(zs_ctx *ctx, uint64_t *member_first, uint32_t *member_in, uint32_t *member_out, uint64_t cap);

/* BGZF files (bgzip output, BAM, tabix-indexed VCF; the SAM specification, section 4.1): the _members entries
 * with the members SIZED FROM THEIR HEADERS where those can be trusted.  A BGZF block states in its header
 * where it ends (BSIZE) and in its trailer how many bytes it produces (ISIZE); the _members entries decode
 * every member once, without storing, to find both.  A header that lies would change their results, so this is
 * a mode with its own entries; the _members entries stay as they are.  gzip only.
 *  - Entries: EXACTLY the arguments of the _members entries.  Refusals are theirs and in their order, before
 *    the context is looked at: wbits other than 31, a null out_cap, the device entry's alignment.  The
 *    candidate cap is the same.
 *  - The header at start p of stream s[0..n) is TRUSTED when all of these hold: p + 18 <= n and s[p..p+4) is
 *    1f 8b 08 04 (FLG exactly 4: FEXTRA alone, as the specification writes it); XLEN (u16 at p + 10) has
 *    p + 12 + XLEN <= n; the subfields (SI1 SI2 SLEN data) tile the XLEN bytes exactly; one subfield is 'B' 'C'
 *    with SLEN 2, the first such one giving BSIZE (it need not be the first subfield); with total = BSIZE + 1,
 *    total > 12 + XLEN + 8 (at least one byte of deflate data) and p + total <= n; ISIZE (u32 at
 *    p + total - 4) <= 65536.  A trusted start is a member of total bytes that produces ISIZE bytes, and no
 *    byte of its deflate data is read to say so.  EVERY OTHER start -- a plain gzip member, an FNAME flag, a
 *    truncated block, a BSIZE that does not fit, a false candidate -- is sized from the data exactly as in the
 *    _members entries, so mixed files, `cat a.gz b.bgz`, trailing bytes and truncation behave as there.
 *  - Well-formed input: for every stream whose trusted headers tell the truth -- any gzip file, BGZF or not --
 *    every field equals the _members entry's: the output, out_len, consumed, status, phase, msg and check,
 *    failures included (a corrupt member, truncation, capacity).
 *  - Lying headers: where a trusted header lies, member k decodes from its BSIZE + 1 bytes into ISIZE bytes of
 *    room.  The stream reports for k what zs_inflate_batch_ex with inflate_ref_wrap = 0 reports for those
 *    bytes alone, with one mapping: a trusted member that was given its ISIZE for room and ends with the
 *    capacity outcome (ZS_BUF_ERROR, "output capacity exceeded") produced more than its ISIZE says and is
 *    reported as ZS_DATA_ERROR, ZS_PHASE_PROCESS, "incorrect length check" (zlib's words for an ISIZE that
 *    does not match), so that a caller can tell it from a capacity of their own that is too small.  (The
 *    first member that does not fit the stream's out_cap is given no room, is not such a member and reports
 *    the capacity outcome, as in _members.  An ISIZE that is too large is the decoder's own "incorrect length
 *    check"; a BSIZE that is too small is input that ends early, ZS_BUF_ERROR without a message.)
 *    out_len[i] = out_pos_k, consumed[i] = start_k, check[i] = 0; the complete members before k are valid, as
 *    in _members; one failed stream does not touch its neighbours; no store leaves a stream's region rounded
 *    up to 4.  NOT verified: a BSIZE that is too large and still fits the input ends member k cleanly (the
 *    plain entry ignores the bytes behind a member) and the chain goes on at p + BSIZE + 1, where it ends
 *    unless those bytes pass the four-byte test: the stream reports success with the members up to k.
 *  - zs_last_members answers after a _bgzf call as after a _members call.
 *  - zs_last_bgzf_trusted(ctx): for tests and tuning, the number of planned members of the last _bgzf call
 *    on the context whose size came from their header; 0 after any other inflate call.  It is known when
 *    the call returns (the plan is made on the host).  Not offered on the pool.
 *  - zs_bgzf_out_len: host arithmetic, needs no context.  It follows trusted headers from offset 0 by the
 *    members' ending rule (the chain ends where the four-byte test fails or the input ends); returns 1 and
 *    writes the sum of ISIZE to *total when every member on the chain is trusted, 0 (and *total = 0) when
 *    the chain meets an untrusted member -- so for an empty input, whose offset 0 is one.  The capacity a
 *    truthful BGZF file needs.
 *  - The DEVICE entry synchronises hip_stream as the _members entry does; a trusted member never needs a
 *    tail round, whatever its data holds.  The HOST entries run as one chunk (zs_last_host_chunks = 1).
 *  - Timing phases: "members_scan", "bgzf_size" (the sizing launch; a tail round stays "members_size") and
 *    "members_stitch", around the decoders' own.
 *  - A range of blocks (a seek by virtual offset) is the _bgzf_range entries' (below); a BGZF writer is
 *    zs_deflate_batch_bgzf*.
 *  - Not built: _auto entries (Python and JS size the output with zs_bgzf_out_len); the chunked host pipeline
 *    (one chunk, as _members). */
int zs_inflate_batch_bgzf_device(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                 const uint64_t *in_off, const uint32_t *in_len, uint8_t *d_out,
                                 const uint64_t *out_off, const uint32_t *out_cap, int32_t *d_status,
                                 int32_t *d_phase, int32_t *d_msg, uint32_t *d_out_len, uint32_t *d_consumed,
                                 uint32_t *d_check, void *hip_stream);
int zs_inflate_batch_bgzf(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                          int32_t *status, int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed,
                          uint32_t *check);
int zs_pool_inflate_batch_bgzf(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in,
                               const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                               const uint32_t *out_cap, int32_t *status, int32_t *phase, int32_t *msg,
                               uint32_t *out_len, uint32_t *consumed, uint32_t *check);
uint64_t zs_last_bgzf_trusted(zs_ctx *ctx);
int zs_bgzf_out_len(const uint8_t *in, uint32_t in_len, uint64_t *total);

/* BGZF ranges by virtual offset: random access, what BGZF exists for (the SAM specification, section 4.1.1).  A
 * virtual offset is coffset << 16 | uoffset: coffset the start of a block in the compressed file, uoffset a
 * position in that block's data.  Every .bai, .tbi and .csi index consists of pairs of them; a region query is
 * "the bytes between these two virtual offsets".  These entries take the _bgzf entries' arguments plus two HOST
 * arrays of n_streams virtual offsets behind in_len.
 *  - Stream i is a BGZF file, or any piece of one that starts at a block; coffset counts from in_off[i].  SEVERAL
 *    STREAMS MAY NAME THE SAME INPUT BYTES: the input is only read, so thousands of region queries over one file
 *    are one call.  The host entries stage only each range's slice of its stream.
 *  - With cb, ub = voff_begin[i] >> 16, & 0xffff and ce, ue likewise: the chain starts at cb and follows trusted
 *    headers (the _bgzf entries' rule, unchanged) while the start is < ce; it must land on ce exactly.  The
 *    decoded members are those with a start in [cb, ce), plus the member at ce when ue > 0, whose header must
 *    then be trusted.  The output is out(m_0)[ub:] | out(m_1) | ... | out(m_e)[:ue]; with cb == ce it is
 *    out(m_0)[ub:ue].  ub == ISIZE is legal and contributes nothing.  With ue == 0 the block at ce is neither
 *    required nor decoded, so ce == in_len[i] is legal; voff_begin == voff_end with ue == 0 decodes nothing and
 *    succeeds with out_len 0, consumed = cb, check 0.
 *  - Success: ZS_STREAM_END; out_len the delivered length; consumed the offset (from the stream's start) behind
 *    the last decoded member, or ce when none follows; check the crc32 of the delivered bytes.  Whole blocks are
 *    decoded, so every decoded block's own CRC32 and ISIZE are still verified.
 *  - Refusals of the whole call (ZS_STREAM_ERROR): the _bgzf entries' in their order; then, still before the
 *    context is looked at, a null voff_begin or voff_end ("null virtual offset arrays"), voff_begin[i] >
 *    voff_end[i] ("a range's begin lies behind its end"), ce > in_len[i] ("a range's end lies past the stream's
 *    input").  The candidate and segment caps are those of the _members entries, over the ranges' slices.
 *  - Failures found from the headers, before anything of that stream decodes: an untrusted header at a chain
 *    start (so cb in the middle of a block), a chain that steps over ce, ub or ue above that block's ISIZE.  The
 *    stream reports ZS_DATA_ERROR, ZS_PHASE_PROCESS, "virtual offsets do not follow a chain of BGZF blocks",
 *    out_len 0, consumed = the offending start, check 0; its region is untouched.
 *    The message has index 23: zs_inflate_message(22), the index behind the restart entries' message, stays the
 *    empty string, which existing callers may test for.
 *  - Capacity is known from the headers: the members before the first whose clipped piece does not fit are
 *    decoded and delivered, and the stream reports what the _bgzf entries report for a total that passes
 *    out_cap; out_len the delivered length, consumed that member's start, check 0.
 *  - Decoder failures and lying headers follow the _bgzf entries' contract for member k, its mapping of the
 *    capacity outcome to "incorrect length check" included; out_len the delivered bytes of the complete members
 *    before k, clipped; consumed = start_k; check 0.
 *  - One failed stream does not touch its neighbours; no store leaves [out_off, out_off + out_cap) rounded up to
 *    4, and none touches a byte of the region behind the delivered length rounded up to 4.
 *  - For a truthful stream that is BGZF throughout (zs_bgzf_out_len answers 1) the range (0, consumed_full << 16),
 *    consumed_full being what the _bgzf entry reports, equals that entry's result in every field.  A stream with
 *    another kind of member on the chain (a plain gzip member, a name in the header, BSIZE 0) fails at that member,
 *    by the chain rule above; the _bgzf entries read such files.
 *  - zs_bgzf_range_out_len: host arithmetic over the same rule, no context: 1 and the delivered length, or 0 (and
 *    *total = 0) where the headers fail the stream or the range is refused.
 *  - zs_bgzf_voffset: an uncompressed position's virtual offset from one stream's index, `count` entries in
 *    increasing order, the end entry included where present: block_in the blocks' offsets in the COMPRESSED
 *    file, block_out their offsets in the uncompressed data -- zs_last_members' member_in and member_out; of
 *    zs_last_bgzf_blocks, whose input is the uncompressed side, block_out and block_in in this order.  It takes
 *    the last block with block_out <= upos.  0 when upos lies behind the last entry (or in front of the first)
 *    or the difference does not fit 16 bits.
 *  - The DEVICE entry synchronises hip_stream as the _bgzf entry does, and once more in front of that where a
 *    range ends inside a block (ue > 0): the header of the block at ce is read first, so that the bytes behind
 *    that block are not searched.  The HOST entries run as one chunk.
 *  - Timing phases: the _bgzf entries', "bgzf_range_end" (the kernel that reads the end blocks' headers),
 *    "bgzf_range_wait" (the host's wait for it, up to the scan) and "bgzf_range_place".  zs_last_bgzf_trusted counts the planned blocks;
 *    zs_last_members does not answer after these entries.
 *  - Not built: de-duplicating blocks shared by overlapping ranges of one call; parsing .bai / .tbi / .csi /
 *    .gzi files; ranges over non-BGZF multi-member gzip or over restart points; _auto entries. */
int zs_inflate_batch_bgzf_range_device(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *d_in,
                                       const uint64_t *in_off, const uint32_t *in_len, const uint64_t *voff_begin,
                                       const uint64_t *voff_end, uint8_t *d_out, const uint64_t *out_off,
                                       const uint32_t *out_cap, int32_t *d_status, int32_t *d_phase, int32_t *d_msg,
                                       uint32_t *d_out_len, uint32_t *d_consumed, uint32_t *d_check, void *hip_stream);
int zs_inflate_batch_bgzf_range(zs_ctx *ctx, int wbits, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                                const uint32_t *in_len, const uint64_t *voff_begin, const uint64_t *voff_end,
                                uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, int32_t *status,
                                int32_t *phase, int32_t *msg, uint32_t *out_len, uint32_t *consumed, uint32_t *check);
int zs_pool_inflate_batch_bgzf_range(zs_pool *pool, int wbits, uint32_t n_streams, const uint8_t *in,
                                     const uint64_t *in_off, const uint32_t *in_len, const uint64_t *voff_begin,
                                     const uint64_t *voff_end, uint8_t *out, const uint64_t *out_off,
                                     const uint32_t *out_cap, int32_t *status, int32_t *phase, int32_t *msg,
                                     uint32_t *out_len, uint32_t *consumed, uint32_t *check);
int zs_bgzf_range_out_len(const uint8_t *in, uint32_t in_len, uint64_t voff_begin, uint64_t voff_end, uint64_t *total);
int zs_bgzf_voffset(const uint32_t *block_in, const uint32_t *block_out, uint64_t count, uint64_t upos, uint64_t *voff);

/* The z_stream message for a d_msg index (inflate.ts:397-1031, inffast.ts:108,197,210). */
const char *zs_inflate_message(int32_t msg_index);

/* Per-stream checksums, check[i] = crc32(seeds[i], in[i]) / adler32(seeds[i], in[i])
 * with the reference's semantics (common/crc32.ts:26-58, common/adler32.ts:4-25):
 * the seed is a running checksum being continued; an empty stream returns the
 * seed unchanged.  seeds: host array of n_streams values, or NULL for the
 * initial values (crc32 0, adler32 1).  The _device forms take device buffers
 * and write d_check on the device (asynchronously on hip_stream); the host forms
 * take host buffers and return when check[] is filled. */
int zs_crc32_batch_device(zs_ctx *ctx, uint32_t n_streams, const uint8_t *d_in, const uint64_t *in_off,
                          const uint32_t *in_len, const uint32_t *seeds, uint32_t *d_check, void *hip_stream);
int zs_adler32_batch_device(zs_ctx *ctx, uint32_t n_streams, const uint8_t *d_in, const uint64_t *in_off,
                            const uint32_t *in_len, const uint32_t *seeds, uint32_t *d_check, void *hip_stream);
int zs_crc32_batch(zs_ctx *ctx, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                   const uint32_t *in_len, const uint32_t *seeds, uint32_t *check);
int zs_adler32_batch(zs_ctx *ctx, uint32_t n_streams, const uint8_t *in, const uint64_t *in_off,
                     const uint32_t *in_len, const uint32_t *seeds, uint32_t *check);
/* Joins the checksums of two pieces: the crc32 / adler32 of A followed by B from
 * crc32(A), crc32(B) and B's length len2 (adler32: from reduced values, as every
 * entry here returns them for a non-empty piece).  len2 == 0 returns the first
 * value.  For pieces checksummed in several calls, contexts or devices (the
 * seeds above continue one piece after the other; these need no order).  Host
 * arithmetic, no context.  No reference counterpart: zlib's crc32_combine /
 * adler32_combine. */
uint32_t zs_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);
uint32_t zs_adler32_combine(uint32_t adler1, uint32_t adler2, uint64_t len2);

/* Kernel timing of the batch calls made on this context since the last query
 * (HIP events on the streams the kernels ran on; the calls themselves never
 * wait for them, the query does): device milliseconds from the first call's
 * start to the last call's end, and the summed duration of the named phase
 * ("sweep", "parse", "trees", "emit", "fast", "inflate_lane", ...).  Returns -1
 * when no timing is available. */
double zs_last_batch_ms(zs_ctx *ctx);
/* Members of the last inflate batch that the lane-per-member path decoded
 * (the rest went through the exact stream-layer state machine).  Synchronizes
 * the batch's stream.  For tests and tuning. */
uint32_t zs_last_inflate_lane_count(zs_ctx *ctx);
/* Members of the last inflate batch that the segmented decode finished
 * (inflate_seg.hip; the others of its members went on to the wave kernel).
 * Synchronizes.  For tests and tuning. */
uint32_t zs_last_inflate_seg_count(zs_ctx *ctx);
/* Parts of the last batch call's data checksum (the deflate wrappers' check
 * values, the checksum entries, the inflate trailer check): 0 when every
 * stream took one wave, else the parts of option "checksum_part" bytes that
 * the batch was cut into (a host entry's chunks added up).  Known when the
 * call returns; does not synchronize.  For tests and tuning. */
uint32_t zs_last_checksum_parts(zs_ctx *ctx);
/* Chunks of streams that the last host-buffer deflate / inflate call on the
 * context ran as (options "host_chunk_min", "host_pack_min" below): 1 or 4
 * after a host call, 0 after a device call (the checksum entries leave it
 * alone).  Known when the call returns; does not synchronize.  For tests and
 * tuning. */
uint32_t zs_last_host_chunks(zs_ctx *ctx);
double zs_last_phase_ms(zs_ctx *ctx, const char *phase);
void zs_set_timing(zs_ctx *ctx, int on);
/* Engine options: "timing" (0/1, as zs_set_timing); "inflate_fast" (default 1):
 * decode members lane-per-member and re-run only those that do not end cleanly
 * on the exact stream-layer state machine (0: exact path for every member);
 * "check_phases" (default 0): synchronise after every kernel phase and fail
 * with ZS_MEM_ERROR naming the phase whose launch or execution failed;
 * "match_sweep" (default 1): levels 4..9 find matches by a counting sort by
 * hash + lock-step sweep, longer streams in windows of 65,535 positions with a
 * 32 KiB look-back (0: the chain-link + per-tile walk kernels, for every stream
 * -- a cross-check);
 * "lane_block" (default 0 = by batch size;
 * else 1..64, a power of two): members per workgroup of the inflate lane path;
 * "inflate_wave_min" (default 32768; 0 = never): members with more input bytes
 * are "large" and decode beside the lane kernel (side stream): deflate64 (and
 * raw deflate with inflate_ref_wrap 0) by the split decode (inflate_split.hip:
 * cut at block boundaries, pieces in parallel), the other formats one per wave
 * (inflate_wave.hip) or, when a batch has lane_large_min of them or more, one
 * per lane (the lane kernel's large-member instance) -- both track the
 * reference's inflate() calls and so reproduce the window-wrap copy below;
 * "inflate_split" (default 1; 0: large deflate64 members take the wave kernel);
 * "lane_large_min" (default 2304; 0: never): large-member count from which the
 * lanes replace the wave kernel;
 * "parse_waves" (default 0 = two below 2048 streams, else one; 1, 2 or 4):
 * waves per stream of the levels 4..9 lazy parse (two: 512-position segments,
 * two rounds' speculative passes at once);
 * "fast_group" (default 1): levels 1..3 replay deflate_fast a group of 64
 * positions at a time from speculative per-lane chain walks (0: step by step);
 * "lane_order" (default 1 when the self-test passes, else 0 and 1 is refused):
 * the chain builders rank equal hashes by same-address LDS atomics applying in
 * lane order (1) or by ballots (0);
 * "inflate_seg" (default 1): batches of at most "seg_small_batch" (default
 * 16,384) members decode every member with more than "seg_small_min" (default
 * 4096) input bytes -- and, in any batch, every member over inflate_wave_min --
 * by the segmented decode (inflate_seg.hip: blocks walked in order, each cut
 * across 64 lanes, the reference's calls tracked per piece); large deflate64
 * members and high-expansion members (cap > 64 KiB, >= 8 output bytes per
 * input byte) take the split / wave decoders instead; "seg_bits" (1024..8192,
 * default 0 = 4096 for members of >= 64 KiB of input on average, else 2048):
 * input bits per lane of an entry's first block; "seg_wide"
 * (default 1): the 2048-bit sync window for a batch of few large members;
 * "seg_split" (0 off, 1 on, default 2 = batches of at most 2 large members per CU):
 * each piece is cut in two at the first symbol start past its lane's middle, so
 * the decode runs twice the pieces, each half as long;
 * "seg_big_bits" (>= 65536, default 2^21): members with more input bits also
 * walk from the block starts a finder kernel proposes (more walks per member);
 * "seg_scratch_mb" (default 16384): the segmented decode's u16 scratch per
 * batch (2 bytes per byte of capacity); members past it take the other paths;
 * "checksum_split" (bytes, default 262144; 0 = never): a batch with a stream
 * longer than this computes its data checksums (gzip / zlib check values, the
 * checksum entries, the inflate trailer check) in parts of "checksum_part"
 * bytes (a power of two 1024 .. 1048576, default 65536), a wave per part, and
 * joins them per stream; other batches take one wave per stream;
 * "host_chunk_min" (bytes, default 33554432; 0 = never): a host-buffer batch
 * of at least 64 streams and this many input bytes runs as four chunks of
 * streams, cut at n/8, 4n/8 and 7n/8, whose staging, kernels and copies back
 * overlap (other batches: one chunk); "host_pack_min" (bytes, default
 * 67108864): the floor of the first size of the host entries' packed-output
 * buffers, min(capacities, max(4 x input, host_pack_min)), which grow when a
 * chunk's output does not fit.
 * These options never change output bytes or check values.  "inflate_ref_wrap" (default 1)
 * does: 1 reproduces the reference's inflate_fast window-wrap copy
 * (inffast.ts:133-147), which changes the output of members whose match
 * crosses the reference's window wrap between inflate() calls; 0 decodes with
 * zlib semantics (the bytes the compressor was given).  "rle_ref" (default 1)
 * does too, for ZS_RLE alone: 1 reproduces the reference's deflate_rle, which
 * finds no run (deflate.ts:1469-1481) and so writes ZS_HUFFMAN_ONLY's bytes; 0
 * compresses as zlib's deflate_rle does (greedy matches at distance 1). */
int zs_set_option(zs_ctx *ctx, const char *name, int value);

/* Introspection for tests: copy an intermediate array of stream s of the last
 * deflate batch to host memory (what: 0 chain links u16/position, 1 match table
 * u32x2/position, 2 symbols u32, 3 block records, 4 stream record).  Returns
 * the bytes copied (0 if unavailable).  Synchronizes the device. */
uint64_t zs_debug_fetch(zs_ctx *ctx, int what, uint32_t s, void *dst, uint64_t cap);

/* Synthetic workload: kind 0 = T-corpus text,
 * 1 = M-corpus mixed, 2 = xorshift bytes; stream i uses seed
 * 0x9e3779b9 ^ (first_index + i).  Fills host memory with n_streams x len. */
void zs_corpus(int kind, uint32_t first_index, uint32_t n_streams, uint32_t len, uint8_t *out, int threads);

#ifdef __cplusplus
}
#endif
#endif
