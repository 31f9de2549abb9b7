/*
 * zsnapi.c -- the thin N-API addon between the JavaScript host side
 * (streams-api.mjs) and libzsgpu.so (include/zs_gpu.h).  Plain C against
 * node_api.h (N-API v8): it reads the callers' Uint8Array backing stores for
 * the duration of one call (napi_get_typedarray_info, SURVEY.md 8(b)
 * "Ownership"), copies them into one buffer the batch owns before the call
 * returns (the caller may then modify, transfer or detach its buffers: N-API
 * cannot pin an ArrayBuffer), hands that to zs_deflate_batch /
 * zs_inflate_batch on the worker thread, and returns the outputs as views of ONE external ArrayBuffer that the batch's
 * output buffer becomes (freed when the views are collected: no copy back
 * either).  The batch calls return Promises: the GPU work runs on a libuv
 * worker thread (napi_async_work), so the event loop keeps running.  A batch
 * runs on a device set (SURVEY.md 8(b) "device mask"): a zs_pool per distinct
 * set, created lazily on the JS thread, splits it into contiguous stream
 * ranges with one host thread per GPU (so an 8-GPU batch is not capped by
 * libuv's 4-thread pool); batches on one set are serialized by the pool.
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/zs_gpu.h"

#define MAX_DEV 64
static zs_ctx *g_ctx[MAX_DEV]; /* selfTest only */

#define MAX_POOLS 64
static struct {
  uint64_t mask;
  zs_pool *pool;
} g_pools[MAX_POOLS];
static int g_npools;

#define NAPI_OK(call)                                      \
  do {                                                     \
    if ((call) != napi_ok) {                               \
      napi_throw_error(env, NULL, "N-API call failed: " #call); \
      return NULL;                                         \
    }                                                      \
  } while (0)

static napi_value throw_code(napi_env env, int code, const char *msg) {
  char c[16];
  snprintf(c, sizeof c, "%d", code);
  napi_throw_error(env, c, msg);
  return NULL;
}

static void throw_unavailable(napi_env env) {
  /* no device / self-test failure: the engine is unavailable, never a CPU fallback */
  char m[600];
  snprintf(m, sizeof m, "MI355X engine unavailable: %s", zs_last_error());
  napi_throw_error(env, "ZS_UNAVAILABLE", m);
}

static zs_ctx *ctx_for(napi_env env, int dev) {
  if (dev < 0 || dev >= MAX_DEV) {
    throw_code(env, ZS_STREAM_ERROR, "device index out of range");
    return NULL;
  }
  if (!g_ctx[dev]) {
    zs_ctx *c = NULL;
    if (zs_ctx_create(dev, &c) != ZS_OK) {
      throw_unavailable(env);
      return NULL;
    }
    g_ctx[dev] = c;
  }
  return g_ctx[dev];
}

/* device spec: a device index, an array of them, or undefined (device 0) -> bit mask;
 * 0 on an invalid spec (a JS exception is pending) */
static uint64_t device_mask(napi_env env, napi_value v) {
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok) return 0;
  if (t == napi_undefined || t == napi_null) return 1;
  bool arr = false;
  napi_is_array(env, v, &arr);
  uint32_t n = 1;
  if (arr) napi_get_array_length(env, v, &n);
  uint64_t m = 0;
  for (uint32_t i = 0; i < n; i++) {
    napi_value e = v;
    if (arr) napi_get_element(env, v, i, &e);
    napi_valuetype et;
    int32_t d = -1;
    if (napi_typeof(env, e, &et) == napi_ok && et == napi_number) napi_get_value_int32(env, e, &d);
    if (d < 0 || d >= MAX_DEV) {
      napi_throw_error(env, "ZS_BAD_DEVICE", "devices must be GPU indices in 0..63");
      return 0;
    }
    m |= 1ull << d;
  }
  if (!m) napi_throw_error(env, "ZS_BAD_DEVICE", "devices must name at least one GPU");
  return m;
}

static zs_pool *pool_for(napi_env env, uint64_t mask) {
  for (int i = 0; i < g_npools; i++)
    if (g_pools[i].mask == mask) return g_pools[i].pool;
  if (g_npools == MAX_POOLS) {
    napi_throw_error(env, "ZS_BAD_DEVICE", "too many distinct device sets");
    return NULL;
  }
  zs_pool *p = NULL;
  const int r = zs_pool_create(mask, &p);
  if (r != ZS_OK) {
    if (r == ZS_STREAM_ERROR && strstr(zs_last_error(), "device mask")) napi_throw_error(env, "ZS_BAD_DEVICE", zs_last_error());
    else throw_unavailable(env);
    return NULL;
  }
  g_pools[g_npools].mask = mask;
  g_pools[g_npools].pool = p;
  g_npools++;
  return p;
}

/* Borrowed view of one input. */
typedef struct {
  const uint8_t *p;
  size_t n;
} view;

static int get_views(napi_env env, napi_value arr, view **out, uint32_t *count) {
  bool is_arr = false;
  if (napi_is_array(env, arr, &is_arr) != napi_ok || !is_arr) return -1;
  uint32_t n = 0;
  if (napi_get_array_length(env, arr, &n) != napi_ok) return -1;
  view *v = (view *)calloc(n ? n : 1, sizeof(view));
  if (!v) return -1;
  for (uint32_t i = 0; i < n; i++) {
    napi_value e;
    bool is_ta = false;
    napi_typedarray_type t;
    size_t len = 0, off = 0;
    void *data = NULL;
    napi_value ab;
    if (napi_get_element(env, arr, i, &e) != napi_ok || napi_is_typedarray(env, e, &is_ta) != napi_ok || !is_ta ||
        napi_get_typedarray_info(env, e, &t, &len, &data, &ab, &off) != napi_ok || t != napi_uint8_array) {
      free(v);
      return -2;
    }
    v[i].p = (const uint8_t *)data;
    v[i].n = len;
  }
  *out = v;
  *count = n;
  return 0;
}

static napi_value make_u8(napi_env env, const uint8_t *src, size_t n) {
  void *data = NULL;
  napi_value ab, ta;
  if (napi_create_arraybuffer(env, n, &data, &ab) != napi_ok) return NULL;
  if (n) memcpy(data, src, n);
  if (napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta) != napi_ok) return NULL;
  return ta;
}

static napi_value make_32(napi_env env, const void *src, size_t n, napi_typedarray_type type) {
  void *data = NULL;
  napi_value ab, ta;
  if (napi_create_arraybuffer(env, 4 * n, &data, &ab) != napi_ok) return NULL;
  if (n) memcpy(data, src, 4 * n);
  if (napi_create_typedarray(env, type, n, ab, 0, &ta) != napi_ok) return NULL;
  return ta;
}
#define make_i32(env, src, n) make_32(env, src, n, napi_int32_array)
#define make_u32(env, src, n) make_32(env, src, n, napi_uint32_array)

/* an output capacity: a number clamped to 0 .. 4 GiB - 4 (the ABI's u32 lengths) */
static uint32_t arg_cap(napi_env env, napi_value v, uint32_t dflt) {
  napi_valuetype t;
  double x = dflt;
  if (napi_typeof(env, v, &t) == napi_ok && t == napi_number) napi_get_value_double(env, v, &x);
  if (!(x > 0)) return 0;
  if (x > 4294967292.0) x = 4294967292.0;
  return (uint32_t)x;
}

static int32_t arg_i32(napi_env env, napi_value v, int32_t dflt) {
  napi_valuetype t;
  int32_t x = dflt;
  if (napi_typeof(env, v, &t) == napi_ok && t == napi_number) napi_get_value_int32(env, v, &x);
  return x;
}

/* One batch in flight: a copy of the inputs taken on the JS thread when the
 * call is made (the caller may modify, transfer or detach its buffers right
 * after: N-API cannot pin an ArrayBuffer's memory), the GPU work on a libuv
 * worker thread (napi_async_work), results built back on the JS thread. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  int inflate;   /* 0 compress, 1 decompress */
  int unbounded; /* decompress without a caller capacity: zs_pool_inflate_batch_auto */
  int wbits, level;
  int strategy;  /* compress: deflateInit2_'s strategy (zs_pool_deflate_batch_strategy when not 0) */
  int params;    /* compress: windowBits / memLevel other than 15 / 8 (zs_pool_deflate_batch_params): wbits is */
  int mem_level; /* deflateInit2_'s windowBits argument then (-9..-15, 8..15, 25..31) */
  uint32_t n;
  zs_pool *pool;
  uint64_t *in_off, *out_off;
  uint32_t *in_len, *cap, *olen, *cons, *check;
  int32_t *status, *phase, *msg;
  uint8_t *base;       /* inputs: base + in_off[i] (the job's own copy) */
  /* preset dictionaries (zs_pool_inflate_batch_dict*, zs_pool_deflate_batch_dict): the job's copy of the
   * distinct ones, input i's at dict + dict_off[i], dict_len[i] bytes (0: none); NULL: none given */
  uint8_t *dict;
  uint64_t *dict_off;
  uint32_t *dict_len;
  /* Z_FULL_FLUSH points (zs_pool_deflate_batch_flush): input i's positions are flush_pos[flush_first[i] ..
   * flush_first[i + 1]); NULL: none given */
  uint64_t *flush_first;
  uint32_t *flush_pos;
  int primed;          /* compress, with flush_first: primed pieces, no flush (zs_pool_deflate_batch_primed) */
  int bgzf;            /* compress: a BGZF file per input (zs_pool_deflate_batch_bgzf) ... */
  uint32_t block_bytes;  /* ... in blocks of this many bytes (0: ZS_BGZF_BLOCK) */
  /* restart points (zs_pool_inflate_batch_restart): input i's points, its start included, are
   * (restart_in[k], restart_out[k]) for k in restart_first[i] .. restart_first[i + 1]; NULL: none given */
  uint64_t *restart_first;
  uint32_t *restart_in, *restart_out;
  int restart_scan;    /* restart "scan": the points are found from the bytes (zs_pool_inflate_batch_sync) */
  int members;         /* restart "members": every member of multi-member gzip inputs (zs_pool_inflate_batch_members);
                          2 = restart "bgzf": BGZF blocks sized from their headers (zs_pool_inflate_batch_bgzf) */
  /* restart "bgzf" with ranges (zs_pool_inflate_batch_bgzf_range): input i's virtual offsets; NULL: none given */
  uint64_t *voff_begin, *voff_end;
  uint8_t *out;
  int out_given;       /* out now belongs to the results' external ArrayBuffer */
  int rc;
  char err[512];
} job;

static void job_free(job *j) {
  if (!j) return;
  free(j->in_off); free(j->out_off); free(j->in_len); free(j->cap); free(j->olen); free(j->cons); free(j->check);
  free(j->status); free(j->phase); free(j->msg); free(j->base);
  free(j->dict); free(j->dict_off); free(j->dict_len);
  free(j->flush_first); free(j->flush_pos);
  free(j->restart_first); free(j->restart_in); free(j->restart_out);
  free(j->voff_begin); free(j->voff_end);
  if (!j->out_given) {
    if (j->unbounded) zs_free(j->out);
    else free(j->out);
  }
  free(j);
}

static job *job_new(uint32_t n) {
  job *j = (job *)calloc(1, sizeof(job));
  if (!j) return NULL;
  j->n = n;
  j->in_off = (uint64_t *)calloc(n + 1, 8);
  j->out_off = (uint64_t *)calloc(n + 1, 8);
  j->in_len = (uint32_t *)calloc(n + 1, 4);
  j->cap = (uint32_t *)calloc(n + 1, 4);
  j->olen = (uint32_t *)calloc(n + 1, 4);
  j->cons = (uint32_t *)calloc(n + 1, 4);
  j->check = (uint32_t *)calloc(n + 1, 4);
  j->status = (int32_t *)calloc(n + 1, 4);
  j->phase = (int32_t *)calloc(n + 1, 4);
  j->msg = (int32_t *)calloc(n + 1, 4);
  if (!j->in_off || !j->out_off || !j->in_len || !j->cap || !j->olen || !j->cons || !j->check || !j->status ||
      !j->phase || !j->msg) {
    job_free(j);
    return NULL;
  }
  return j;
}

/* worker thread: no N-API calls here */
static void job_execute(napi_env env, void *data) {
  job *j = (job *)data;
  (void)env;
  if (j->n == 0) j->rc = ZS_OK;
  else if (j->inflate && j->dict_off && j->unbounded)
    j->rc = zs_pool_inflate_batch_dict_auto(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, &j->out,
                                            j->out_off, j->status, j->phase, j->msg, j->olen, j->cons, j->check,
                                            j->dict, j->dict_off, j->dict_len);
  else if (j->inflate && j->dict_off)
    j->rc = zs_pool_inflate_batch_dict(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out, j->out_off,
                                       j->cap, j->status, j->phase, j->msg, j->olen, j->cons, j->check, j->dict,
                                       j->dict_off, j->dict_len);
  else if (j->inflate && j->members == 2 && j->voff_begin)
    j->rc = zs_pool_inflate_batch_bgzf_range(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, j->voff_begin,
                                             j->voff_end, j->out, j->out_off, j->cap, j->status, j->phase, j->msg, j->olen,
                                             j->cons, j->check);
  else if (j->inflate && j->members == 2)
    j->rc = zs_pool_inflate_batch_bgzf(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out, j->out_off, j->cap,
                                       j->status, j->phase, j->msg, j->olen, j->cons, j->check);
  else if (j->inflate && j->members)
    j->rc = zs_pool_inflate_batch_members(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out, j->out_off,
                                          j->cap, j->status, j->phase, j->msg, j->olen, j->cons, j->check);
  else if (j->inflate && j->restart_scan)
    j->rc = zs_pool_inflate_batch_sync(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out, j->out_off, j->cap,
                                       j->status, j->phase, j->msg, j->olen, j->cons, j->check);
  else if (j->inflate && j->restart_first)
    j->rc = zs_pool_inflate_batch_restart(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out, j->out_off,
                                          j->cap, j->status, j->phase, j->msg, j->olen, j->cons, j->check,
                                          j->restart_first, j->restart_in, j->restart_out);
  else if (j->inflate && j->unbounded)
    j->rc = zs_pool_inflate_batch_auto(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, &j->out, j->out_off,
                                       j->status, j->phase, j->msg, j->olen, j->cons, j->check);
  else if (j->inflate)
    j->rc = zs_pool_inflate_batch(j->pool, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out, j->out_off, j->cap,
                                  j->status, j->phase, j->msg, j->olen, j->cons, j->check);
  else if (j->dict_off)
    j->rc = zs_pool_deflate_batch_dict(j->pool, j->level, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out,
                                       j->out_off, j->cap, j->status, j->olen, j->check, j->dict, j->dict_off,
                                       j->dict_len);
  else if (j->bgzf)
    j->rc = zs_pool_deflate_batch_bgzf(j->pool, j->level, j->n, j->base, j->in_off, j->in_len, j->out, j->out_off,
                                       j->cap, j->status, j->olen, j->check, j->block_bytes);
  else if (j->flush_first && j->primed)
    j->rc = zs_pool_deflate_batch_primed(j->pool, j->level, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out,
                                         j->out_off, j->cap, j->status, j->olen, j->check, j->flush_first, j->flush_pos);
  else if (j->flush_first)
    j->rc = zs_pool_deflate_batch_flush(j->pool, j->level, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out,
                                        j->out_off, j->cap, j->status, j->olen, j->check, ZS_FULL_FLUSH, j->flush_first,
                                        j->flush_pos);
  else if (j->params)
    j->rc = zs_pool_deflate_batch_params(j->pool, j->level, j->wbits, j->mem_level, j->n, j->base, j->in_off, j->in_len,
                                         j->out, j->out_off, j->cap, j->status, j->olen, j->check);
  else if (j->strategy)
    j->rc = zs_pool_deflate_batch_strategy(j->pool, j->level, j->strategy, j->wbits, j->n, j->base, j->in_off, j->in_len,
                                           j->out, j->out_off, j->cap, j->status, j->olen, j->check);
  else
    j->rc = zs_pool_deflate_batch(j->pool, j->level, j->wbits, j->n, j->base, j->in_off, j->in_len, j->out,
                                  j->out_off, j->cap, j->status, j->olen, j->check);
  if (j->rc != ZS_OK) snprintf(j->err, sizeof j->err, "%s", zs_last_error());  /* the error is per thread */
}

static void free_out(napi_env env, void *data, void *hint) {
  (void)env;
  if (hint) zs_free(data);
  else free(data);
}

static napi_value build_result(napi_env env, job *j) {
  napi_value outs, obj;
  if (napi_create_array_with_length(env, j->n, &outs) != napi_ok || napi_create_object(env, &obj) != napi_ok) return NULL;
  napi_value msgs = NULL;
  if (j->inflate && napi_create_array_with_length(env, j->n, &msgs) != napi_ok) return NULL;
  /* the outputs: views of the batch's output buffer, which becomes an external
   * ArrayBuffer (copies only where the runtime refuses external buffers) */
  napi_value ab = NULL;
  uint64_t span = 0;
  for (uint32_t i = 0; i < j->n; i++)
    if (j->status[i] == ZS_STREAM_END && j->out_off[i] + j->olen[i] > span) span = j->out_off[i] + j->olen[i];
  if (j->out && span &&
      napi_create_external_arraybuffer(env, j->out, (size_t)span, free_out, j->unbounded ? (void *)1 : NULL, &ab) ==
          napi_ok)
    j->out_given = 1;
  for (uint32_t i = 0; i < j->n; i++) {
    const size_t len = j->status[i] == ZS_STREAM_END ? j->olen[i] : 0;
    napi_value u = NULL;
    if (ab && len) {
      if (napi_create_typedarray(env, napi_uint8_array, len, ab, (size_t)j->out_off[i], &u) != napi_ok) u = NULL;
    } else {
      u = make_u8(env, j->out ? j->out + j->out_off[i] : NULL, len);
    }
    if (!u || napi_set_element(env, outs, i, u) != napi_ok) return NULL;
    if (j->inflate) {
      napi_value s;
      const char *m = zs_inflate_message(j->msg[i]);
      if (napi_create_string_utf8(env, m ? m : "", NAPI_AUTO_LENGTH, &s) != napi_ok ||
          napi_set_element(env, msgs, i, s) != napi_ok)
        return NULL;
    }
  }
  napi_set_named_property(env, obj, "status", make_i32(env, j->status, j->n));
  napi_set_named_property(env, obj, "check", make_u32(env, j->check, j->n));
  if (j->inflate) {
    napi_set_named_property(env, obj, "phase", make_i32(env, j->phase, j->n));
    napi_set_named_property(env, obj, "consumed", make_i32(env, (const int32_t *)j->cons, j->n));
    napi_set_named_property(env, obj, "message", msgs);
  }
  napi_set_named_property(env, obj, "outputs", outs);
  return obj;
}

/* JS thread: settle the promise */
static void job_complete(napi_env env, napi_status st, void *data) {
  job *j = (job *)data;
  napi_value v = NULL;
  if (st == napi_ok && j->rc == ZS_OK) v = build_result(env, j);
  if (v) {
    napi_resolve_deferred(env, j->deferred, v);
  } else {
    char c[16];
    napi_value code, msg, e;
    const int rc = j->rc != ZS_OK ? j->rc : ZS_MEM_ERROR;
    snprintf(c, sizeof c, "%d", rc);
    napi_create_string_utf8(env, c, NAPI_AUTO_LENGTH, &code);
    napi_create_string_utf8(env, j->rc != ZS_OK ? j->err : "could not build the batch result", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, code, msg, &e);
    napi_reject_deferred(env, j->deferred, e);
  }
  napi_delete_async_work(env, j->work);
  job_free(j);
}

/* the inputs copied, packed, into one buffer the job owns */
static int copy_inputs(job *j, const view *v) {
  uint64_t tot = 0;
  for (uint32_t i = 0; i < j->n; i++) {
    j->in_off[i] = tot;
    j->in_len[i] = (uint32_t)v[i].n;
    tot += v[i].n;
  }
  j->base = (uint8_t *)malloc(tot ? tot : 1);
  if (!j->base) return -1;
  for (uint32_t i = 0; i < j->n; i++)
    if (v[i].n) memcpy(j->base + j->in_off[i], v[i].p, v[i].n);
  return 0;
}

/* copy_inputs for a call with ranges: an input that is the same bytes as the one before it (the same view: many
 * ranges over one file) is copied once */
static int view_same(const view *v, uint32_t i) { return i && v[i].p == v[i - 1].p && v[i].n == v[i - 1].n; }
static int copy_inputs_shared(job *j, const view *v) {
  uint64_t tot = 0;
  for (uint32_t i = 0; i < j->n; i++) {
    const int same = view_same(v, i);
    j->in_off[i] = same ? j->in_off[i - 1] : tot;
    j->in_len[i] = (uint32_t)v[i].n;
    if (!same) tot += v[i].n;
  }
  j->base = (uint8_t *)malloc(tot ? tot : 1);
  if (!j->base) return -1;
  for (uint32_t i = 0; i < j->n; i++)  /* (the same test, not the offsets: an empty input shares its offset with the next) */
    if (v[i].n && !view_same(v, i)) memcpy(j->base + j->in_off[i], v[i].p, v[i].n);
  return 0;
}

/* ranges: [vb, ve][] of BigInt virtual offsets, one pair per input; 0 ok, -1 out of memory, -2 malformed */
static int copy_ranges(napi_env env, job *j, napi_value arr) {
  bool is_arr = false;
  uint32_t len = 0;
  napi_is_array(env, arr, &is_arr);
  if (!is_arr || napi_get_array_length(env, arr, &len) != napi_ok || len != j->n) return -2;
  j->voff_begin = (uint64_t *)calloc(j->n + 1, 8);
  j->voff_end = (uint64_t *)calloc(j->n + 1, 8);
  if (!j->voff_begin || !j->voff_end) return -1;
  for (uint32_t i = 0; i < j->n; i++) {
    napi_value pair, e;
    bool is_pair = false;
    uint32_t two = 0;
    if (napi_get_element(env, arr, i, &pair) != napi_ok) return -2;
    napi_is_array(env, pair, &is_pair);
    if (!is_pair || napi_get_array_length(env, pair, &two) != napi_ok || two != 2) return -2;
    for (uint32_t k = 0; k < 2; k++) {
      bool lossless = false;
      uint64_t x = 0;
      if (napi_get_element(env, pair, k, &e) != napi_ok || napi_get_value_bigint_uint64(env, e, &x, &lossless) != napi_ok ||
          !lossless)
        return -2;
      (k ? j->voff_end : j->voff_begin)[i] = x;
    }
  }
  return 0;
}

static napi_value queue_job(napi_env env, job *j, const char *name) {
  napi_value promise, res_name;
  if (napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &res_name) != napi_ok ||
      napi_create_async_work(env, NULL, res_name, job_execute, job_complete, j, &j->work) != napi_ok ||
      napi_queue_async_work(env, j->work) != napi_ok) {
    job_free(j);
    return throw_code(env, ZS_MEM_ERROR, "could not queue the batch");
  }
  return promise;
}

/* The dictionaries of a job: arr[i] a Uint8Array (input i's preset dictionary) or
 * null / undefined (none).  Copied like the inputs; an object given for several inputs in a
 * row (or among the last few distinct ones) is stored once.  0, -1 out of memory, -2 not views. */
static int copy_dicts(napi_env env, job *j, napi_value arr) {
  enum { RECENT = 16 };
  uint32_t len = 0;
  if (napi_get_array_length(env, arr, &len) != napi_ok || len != j->n) return -2;
  j->dict_off = (uint64_t *)calloc(j->n + 1, 8);
  j->dict_len = (uint32_t *)calloc(j->n + 1, 4);
  view *v = (view *)calloc(j->n + 1, sizeof(view));
  if (!j->dict_off || !j->dict_len || !v) {
    free(v);
    return -1;
  }
  view seen[RECENT];
  uint64_t seen_off[RECENT], tot = 0;
  uint32_t nseen = 0, next = 0;
  int rc = 0;
  for (int pass = 0; pass < 2 && rc == 0; pass++) {
    /* pass 0: views, offsets, the total; pass 1: the copy */
    if (pass == 1) {
      j->dict = (uint8_t *)malloc(tot ? tot : 1);
      if (!j->dict) rc = -1;
    }
    for (uint32_t i = 0; i < j->n && rc == 0; i++) {
      if (pass == 1) {
        if (v[i].n) memcpy(j->dict + j->dict_off[i], v[i].p, v[i].n);
        continue;
      }
      napi_value e;
      napi_valuetype t;
      if (napi_get_element(env, arr, i, &e) != napi_ok || napi_typeof(env, e, &t) != napi_ok) { rc = -2; break; }
      if (t == napi_undefined || t == napi_null) continue;
      bool is_ta = false;
      napi_typedarray_type tt;
      size_t n = 0, off = 0;
      void *data = NULL;
      napi_value ab;
      if (napi_is_typedarray(env, e, &is_ta) != napi_ok || !is_ta ||
          napi_get_typedarray_info(env, e, &tt, &n, &data, &ab, &off) != napi_ok || tt != napi_uint8_array ||
          n > 0xffffffffull) {
        rc = -2;
        break;
      }
      if (!n) continue;
      v[i].p = (const uint8_t *)data;
      v[i].n = n;
      j->dict_len[i] = (uint32_t)n;
      uint32_t k = 0;
      while (k < nseen && !(seen[k].p == v[i].p && seen[k].n == n)) k++;
      if (k < nseen) {
        j->dict_off[i] = seen_off[k];
        v[i].n = 0; /* (stored already: nothing to copy) */
      } else {
        j->dict_off[i] = tot;
        seen[next % RECENT] = v[i]; /* (once full, the oldest slot is reused) */
        seen_off[next % RECENT] = tot;
        next++;
        if (nseen < RECENT) nseen++;
        tot += n;
      }
    }
  }
  free(v);
  return rc;
}

/* The flush positions of a job: arr[i] an array of numbers (input i's Z_FULL_FLUSH positions) or null /
 * undefined (none).  0, -1 out of memory, -2 not such an array.  (The positions' order and range are the
 * entry's to check: "invalid flush positions".) */
static int copy_flush(napi_env env, job *j, napi_value arr) {
  uint32_t len = 0;
  bool is_arr = false;
  if (napi_is_array(env, arr, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, arr, &len) != napi_ok ||
      len != j->n)
    return -2;
  j->flush_first = (uint64_t *)calloc((size_t)j->n + 1, 8);
  if (!j->flush_first) return -1;
  uint64_t tot = 0;
  for (int pass = 0; pass < 2; pass++) {
    /* pass 0: the counts; pass 1: the positions */
    if (pass == 1) {
      j->flush_pos = (uint32_t *)calloc((size_t)tot + 1, 4);
      if (!j->flush_pos) return -1;
    }
    uint64_t at = 0;
    for (uint32_t i = 0; i < j->n; i++) {
      napi_value e;
      napi_valuetype t;
      uint32_t k = 0;
      if (napi_get_element(env, arr, i, &e) != napi_ok || napi_typeof(env, e, &t) != napi_ok) return -2;
      if (t != napi_undefined && t != napi_null) {
        if (napi_is_array(env, e, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, e, &k) != napi_ok)
          return -2;
      }
      if (pass == 0) j->flush_first[i] = at;
      for (uint32_t q = 0; pass == 1 && q < k; q++) {
        napi_value x;
        double d = -1;
        if (napi_get_element(env, e, q, &x) != napi_ok || napi_get_value_double(env, x, &d) != napi_ok ||
            !(d >= 0 && d <= 4294967295.0) || d != (double)(uint32_t)d)
          return -2;
        j->flush_pos[at + q] = (uint32_t)d;
      }
      at += k;
    }
    tot = at;
    j->flush_first[j->n] = tot;
  }
  return 0;
}

/* The restart points of a decompress job: arr[i] a flat array of numbers in0, out0, in1, out1, ... (input i's
 * points, its start first).  0, -1 out of memory, -2 not such an array.  (Their order and range are the
 * entry's to check.) */
static int copy_restart(napi_env env, job *j, napi_value arr) {
  const int rc = copy_flush(env, j, arr);  /* (the same shape: one list of 32-bit values per input) */
  uint64_t *first = j->flush_first;
  uint32_t *flat = j->flush_pos;
  j->flush_first = NULL;
  j->flush_pos = NULL;
  int r = rc;
  if (r == 0) {
    const uint64_t tot = first[j->n];
    for (uint32_t i = 0; i <= j->n && r == 0; i++)
      if (first[i] & 1) r = -2;
    j->restart_in = (uint32_t *)calloc((size_t)tot / 2 + 1, 4);
    j->restart_out = (uint32_t *)calloc((size_t)tot / 2 + 1, 4);
    if (r == 0 && (!j->restart_in || !j->restart_out)) r = -1;
    for (uint64_t k = 0; r == 0 && k < tot / 2; k++) {
      j->restart_in[k] = flat[2 * k];
      j->restart_out[k] = flat[2 * k + 1];
    }
    for (uint32_t i = 0; r == 0 && i <= j->n; i++) first[i] /= 2;
  }
  if (r == 0) {
    j->restart_first = first;
    first = NULL;
  }
  free(first);
  free(flat);
  return r;
}

/* compressBatch(inputs: Uint8Array[], wbits, level, devices: number | number[],
 *               dictionaries: (Uint8Array | null)[] | undefined, strategy: number | undefined,
 *               memLevel: number | undefined, flushAt: (number[] | null)[] | undefined,
 *               bgzf: number | undefined, primed: boolean | undefined) ->
 * primed: true with flushAt: the pieces between the positions are primed with the 32 KiB in front of them and
 * no flush is written (zs_pool_deflate_batch_primed; all three formats); without flushAt, or with bgzf, it
 * throws code "-2", before any device is touched.
 * bgzf: the block's bytes of a BGZF file per input (zs_gpu.h: 0 = 65,280; above that code "-2", "invalid BGZF
 * block size"); wbits must be 31, and together with dictionaries, a strategy, windowBits / memLevel other than
 * 15 / 8 or flushAt it throws code "-2" (not built), before any device is touched.
 * flushAt: Z_FULL_FLUSH positions, one array per input (zs_gpu.h: increasing, at most the input's length;
 * levels 1..9); together with dictionaries, a strategy or windowBits / memLevel other than 15 / 8 it throws
 * code "-2" (not built), before any device is touched.
 * wbits: deflateInit2_'s windowBits argument, -9..-15 / 8..15 / 25..31; memLevel 1..9 (a non-number means 8);
 * anything else throws code "-2" (deflate.ts:281-294), and so does a window other than 15 or a memLevel other
 * than 8 together with dictionaries or a strategy (not built, zs_gpu.h), before any device is touched.
 * strategy: 0..4 (a non-number means 0); out of range, or not 0 together with dictionaries, throws code "-2"
 * (deflate.ts:289-290; no dictionaries with a strategy, zs_gpu.h) before any device is touched ->
 *   Promise<{status: Int32Array, check: Uint32Array, outputs: Uint8Array[]}> */
static napi_value CompressBatch(napi_env env, napi_callback_info info) {
  size_t argc = 10;
  napi_value argv[10];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3)
    return throw_code(env, ZS_STREAM_ERROR,
                      "compressBatch(inputs, wbits, level[, devices[, dictionaries[, strategy[, memLevel[, flushAt[, bgzf[, primed]]]]]]])");
  const int32_t strategy = argc > 5 ? arg_i32(env, argv[5], 0) : 0;
  if (strategy < 0 || strategy > ZS_FIXED) return throw_code(env, ZS_STREAM_ERROR, "invalid strategy");
  napi_valuetype dt = napi_undefined;
  if (argc > 4) napi_typeof(env, argv[4], &dt);
  if (strategy && dt != napi_undefined && dt != napi_null)
    return throw_code(env, ZS_STREAM_ERROR, "a strategy with preset dictionaries is not built");
  const int32_t wbits = arg_i32(env, argv[1], -15), mem_level = argc > 6 ? arg_i32(env, argv[6], 8) : 8;
  {
    const int32_t w = wbits < 0 ? -wbits : wbits > 15 ? wbits - 16 : wbits;  /* deflate.ts:272-294 */
    if (w < 8 || w > 15 || (w == 8 && (wbits < 0 || wbits > 15)))
      return throw_code(env, ZS_STREAM_ERROR, "invalid window bits");
    if (mem_level < 1 || mem_level > 9) return throw_code(env, ZS_STREAM_ERROR, "invalid memLevel");
  }
  const int params = mem_level != 8 || (wbits != -15 && wbits != 15 && wbits != 31);
  if (params && (strategy || (dt != napi_undefined && dt != napi_null)))
    return throw_code(env, ZS_STREAM_ERROR, "windowBits / memLevel with preset dictionaries or a strategy is not built");
  napi_valuetype ft = napi_undefined;
  if (argc > 7) napi_typeof(env, argv[7], &ft);
  const int flush = ft != napi_undefined && ft != napi_null;
  if (flush && (params || strategy || (dt != napi_undefined && dt != napi_null)))
    return throw_code(env, ZS_STREAM_ERROR,
                      "flush points with preset dictionaries, a strategy or windowBits / memLevel are not built");
  napi_valuetype bt = napi_undefined;
  if (argc > 8) napi_typeof(env, argv[8], &bt);
  const int bgzf = bt == napi_number;
  double block = 0;
  if (bgzf) napi_get_value_double(env, argv[8], &block);
  if (bgzf && (wbits != 31 || params || strategy || flush || (dt != napi_undefined && dt != napi_null)))
    return throw_code(env, ZS_STREAM_ERROR,
                      "BGZF is gzip without preset dictionaries, a strategy, windowBits / memLevel or flush points");
  bool primed = false;
  if (argc > 9 && napi_get_value_bool(env, argv[9], &primed) != napi_ok) primed = false;
  if (primed && (!flush || bgzf))
    return throw_code(env, ZS_STREAM_ERROR, "primed pieces need flushAt and are not built with BGZF");
  if (bgzf && !(block >= 0 && block <= ZS_BGZF_BLOCK && block == (double)(uint32_t)block))
    return throw_code(env, ZS_STREAM_ERROR, "invalid BGZF block size");
  view *v = NULL;
  uint32_t n = 0;
  if (get_views(env, argv[0], &v, &n) != 0) return throw_code(env, ZS_STREAM_ERROR, "inputs must be Uint8Array[]");
  napi_value undef;
  napi_get_undefined(env, &undef);
  const uint64_t mask = device_mask(env, argc > 3 ? argv[3] : undef);
  zs_pool *pool = mask ? pool_for(env, mask) : NULL;
  job *j = pool ? job_new(n) : NULL;
  if (!j) {
    free(v);
    return pool ? throw_code(env, ZS_MEM_ERROR, "out of host memory") : NULL;
  }
  j->pool = pool;
  j->wbits = wbits;
  j->level = arg_i32(env, argv[2], -1);
  j->bgzf = bgzf;
  j->primed = primed;
  j->block_bytes = (uint32_t)block;
  j->strategy = strategy;
  j->params = params;
  j->mem_level = mem_level;
  if (dt != napi_undefined && dt != napi_null) {
    bool is_arr = false;
    napi_is_array(env, argv[4], &is_arr);
    const int rc = is_arr ? copy_dicts(env, j, argv[4]) : -2;
    if (rc != 0) {
      free(v);
      job_free(j);
      return rc == -1 ? throw_code(env, ZS_MEM_ERROR, "out of host memory")
                      : throw_code(env, ZS_STREAM_ERROR, "dictionaries must be (Uint8Array | null)[], one per input");
    }
  }
  if (flush) {
    const int rc = copy_flush(env, j, argv[7]);
    if (rc != 0) {
      free(v);
      job_free(j);
      return rc == -1 ? throw_code(env, ZS_MEM_ERROR, "out of host memory")
                      : throw_code(env, ZS_STREAM_ERROR, "flushAt must be (number[] | null)[], one per input");
    }
  }
  uint64_t tout = 0;
  for (uint32_t i = 0; i < n; i++) {
    j->out_off[i] = tout;
    const uint64_t bound = bgzf ? zs_deflate_bound_bgzf(v[i].n, j->block_bytes)
                           : params ? zs_deflate_bound_params(v[i].n, wbits, mem_level, j->level == -1 ? 6 : j->level)
                           : j->flush_first ? zs_deflate_bound_flush(v[i].n, j->wbits, j->flush_first[i + 1] - j->flush_first[i])
                                  : zs_deflate_bound_dict(v[i].n, j->wbits, j->dict_len ? j->dict_len[i] : 0);
    j->cap[i] = (uint32_t)((bound + 3) & ~3ull);
    tout += j->cap[i];
  }
  j->out = (uint8_t *)malloc(tout ? tout : 1);  /* (uninitialised: only the outputs are written) */
  if (!j->out || copy_inputs(j, v) != 0) {
    free(v);
    job_free(j);
    return throw_code(env, ZS_MEM_ERROR, "out of host memory");
  }
  free(v);
  return queue_job(env, j, "zs.compressBatch");
}

/* decompressBatch(inputs: Uint8Array[], wbits, outCapacity: number | number[] | undefined, devices,
 *                 dictionaries: (Uint8Array | null)[] | undefined,
 *                 restart: number[][] | "scan" | "members" | "bgzf" | undefined) ->
 *   Promise<{status, phase: Int32Array, message: string[], outputs: Uint8Array[], consumed: Int32Array,
 *            check: Uint32Array}>
 * outCapacity undefined: unbounded output, as DecompressionStream (zs_pool_inflate_batch_auto).
 * restart: per input the flat pairs in_pos, out_pos of its points, the start first (zs_pool_inflate_batch_restart,
 * zs_gpu.h), or the string "scan": the points are found from the bytes (zs_pool_inflate_batch_sync), or the
 * string "members": every member of multi-member gzip inputs is decoded (zs_pool_inflate_batch_members), or the
 * string "bgzf": the same with BGZF blocks sized from their headers (zs_pool_inflate_batch_bgzf); each
 * needs outCapacity, and together with dictionaries it throws code "-2" (not built), before any device is
 * touched.
 * ranges (a seventh argument, with restart "bgzf" only): [vb, ve][] of BigInt virtual offsets, one pair per input
 * (zs_pool_inflate_batch_bgzf_range); consecutive inputs that are the same view are copied once. */
static napi_value DecompressBatch(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2)
    return throw_code(env, ZS_STREAM_ERROR,
                      "decompressBatch(inputs, wbits[, outCapacity[, devices[, dictionaries[, restart]]]])");
  {
    napi_valuetype rt = napi_undefined, dt0 = napi_undefined, ct0 = napi_undefined;
    if (argc > 5) napi_typeof(env, argv[5], &rt);
    if (argc > 4) napi_typeof(env, argv[4], &dt0);
    if (argc > 2) napi_typeof(env, argv[2], &ct0);
    if (rt != napi_undefined && rt != napi_null &&
        ((dt0 != napi_undefined && dt0 != napi_null) || ct0 == napi_undefined || ct0 == napi_null))
      return throw_code(env, ZS_STREAM_ERROR, "restart points need outCapacity and take no preset dictionaries");
  }
  view *v = NULL;
  uint32_t n = 0;
  if (get_views(env, argv[0], &v, &n) != 0) return throw_code(env, ZS_STREAM_ERROR, "inputs must be Uint8Array[]");
  napi_value undef;
  napi_get_undefined(env, &undef);
  const uint64_t mask = device_mask(env, argc > 3 ? argv[3] : undef);
  zs_pool *pool = mask ? pool_for(env, mask) : NULL;
  job *j = pool ? job_new(n) : NULL;
  if (!j) {
    free(v);
    return pool ? throw_code(env, ZS_MEM_ERROR, "out of host memory") : NULL;
  }
  j->inflate = 1;
  j->pool = pool;
  j->wbits = arg_i32(env, argv[1], -15);
  napi_valuetype ct = napi_undefined;
  if (argc > 2) napi_typeof(env, argv[2], &ct);
  j->unbounded = ct == napi_undefined || ct == napi_null;
  bool caps_arr = false;
  if (!j->unbounded) napi_is_array(env, argv[2], &caps_arr);
  const uint32_t cap_all = caps_arr || j->unbounded ? 0 : arg_cap(env, argv[2], 1 << 16);
  uint64_t tout = 0;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t c = cap_all;
    if (caps_arr) {
      napi_value e;
      napi_get_element(env, argv[2], i, &e);
      c = arg_cap(env, e, 1 << 16);
    }
    j->out_off[i] = tout;
    j->cap[i] = c;  /* exact: Z_BUF_ERROR past it (the host entry stages in word-aligned regions itself) */
    tout += j->cap[i];
  }
  j->out = j->unbounded ? NULL : (uint8_t *)malloc(tout ? tout : 1);  /* unbounded: the library allocates it */
  napi_valuetype gt = napi_undefined;
  if (argc > 6) napi_typeof(env, argv[6], &gt);
  const int ranged = gt != napi_undefined && gt != napi_null;
  if ((!j->unbounded && !j->out) || (ranged ? copy_inputs_shared(j, v) : copy_inputs(j, v)) != 0) {
    free(v);
    job_free(j);
    return throw_code(env, ZS_MEM_ERROR, "out of host memory");
  }
  free(v);
  napi_valuetype dt = napi_undefined;
  if (argc > 4) napi_typeof(env, argv[4], &dt);
  if (dt != napi_undefined && dt != napi_null) {
    bool is_arr = false;
    napi_is_array(env, argv[4], &is_arr);
    const int rc = is_arr ? copy_dicts(env, j, argv[4]) : -2;
    if (rc != 0) {
      job_free(j);
      return rc == -1 ? throw_code(env, ZS_MEM_ERROR, "out of host memory")
                      : throw_code(env, ZS_STREAM_ERROR, "dictionaries must be (Uint8Array | null)[], one per input");
    }
  }
  napi_valuetype rt = napi_undefined;
  if (argc > 5) napi_typeof(env, argv[5], &rt);
  if (rt == napi_string) {
    char word[8] = "";
    size_t len = 0;
    napi_get_value_string_utf8(env, argv[5], word, sizeof word, &len);
    if (strcmp(word, "members") == 0) {
      j->members = 1;
    } else if (strcmp(word, "bgzf") == 0) {
      j->members = 2;
    } else if (strcmp(word, "scan") == 0) {
      j->restart_scan = 1;
    } else {
      job_free(j);
      return throw_code(env, ZS_STREAM_ERROR, "restart must be number[][], \"scan\", \"members\" or \"bgzf\"");
    }
  } else if (rt != napi_undefined && rt != napi_null) {
    const int rc = copy_restart(env, j, argv[5]);
    if (rc != 0) {
      job_free(j);
      return rc == -1 ? throw_code(env, ZS_MEM_ERROR, "out of host memory")
                      : throw_code(env, ZS_STREAM_ERROR, "restart must be number[][]: in_pos, out_pos pairs, one list per input");
    }
  }
  if (ranged) {
    const int rc = j->members == 2 ? copy_ranges(env, j, argv[6]) : -3;
    if (rc != 0) {
      job_free(j);
      return rc == -1   ? throw_code(env, ZS_MEM_ERROR, "out of host memory")
             : rc == -3 ? throw_code(env, ZS_STREAM_ERROR, "ranges need restart \"bgzf\"")
                        : throw_code(env, ZS_STREAM_ERROR, "ranges must be [vb, ve][] of BigInt, one pair per input");
    }
  }
  return queue_job(env, j, "zs.decompressBatch");
}

static napi_value DeflateBound(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2], r;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  double len = 0;
  napi_get_value_double(env, argv[0], &len);
  NAPI_OK(napi_create_double(env, (double)zs_deflate_bound((uint64_t)len, argc > 1 ? arg_i32(env, argv[1], -15) : -15), &r));
  return r;
}

/* bgzfOutLength(input: Uint8Array) -> number: the bytes a BGZF file produces, read from its headers
 * (zs_bgzf_out_len: host arithmetic), or -1 when a member on the way is no BGZF block whose header can be trusted */
static napi_value BgzfOutLength(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], r;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool is_ta = false;
  if (argc) napi_is_typedarray(env, argv[0], &is_ta);
  napi_typedarray_type type = napi_int8_array;
  size_t len = 0;
  void *data = NULL;
  if (is_ta) napi_get_typedarray_info(env, argv[0], &type, &len, &data, NULL, NULL);
  if (!is_ta || type != napi_uint8_array || len > 0xffffffffu)
    return throw_code(env, ZS_STREAM_ERROR, "bgzfOutLength(input: Uint8Array)");
  uint64_t total = 0;
  const int ok = len ? zs_bgzf_out_len((const uint8_t *)data, (uint32_t)len, &total) : 0;
  NAPI_OK(napi_create_double(env, ok ? (double)total : -1.0, &r));
  return r;
}

/* bgzfRangeOutLength(input: Uint8Array, vb: bigint, ve: bigint) -> number: the bytes the range between two virtual
 * offsets delivers, read from the headers (zs_bgzf_range_out_len: host arithmetic), or -1 where the offsets do not
 * follow a chain of BGZF blocks */
static napi_value BgzfRangeOutLength(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], r;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool is_ta = false, l0 = false, l1 = false;
  if (argc) napi_is_typedarray(env, argv[0], &is_ta);
  napi_typedarray_type type = napi_int8_array;
  size_t len = 0;
  void *data = NULL;
  uint64_t vb = 0, ve = 0;
  if (is_ta) napi_get_typedarray_info(env, argv[0], &type, &len, &data, NULL, NULL);
  if (!is_ta || type != napi_uint8_array || len > 0xffffffffu || argc < 3 ||
      napi_get_value_bigint_uint64(env, argv[1], &vb, &l0) != napi_ok || !l0 ||
      napi_get_value_bigint_uint64(env, argv[2], &ve, &l1) != napi_ok || !l1)
    return throw_code(env, ZS_STREAM_ERROR, "bgzfRangeOutLength(input: Uint8Array, vb: bigint, ve: bigint)");
  uint64_t total = 0;
  const int ok = zs_bgzf_range_out_len((const uint8_t *)data, (uint32_t)len, vb, ve, &total);
  NAPI_OK(napi_create_double(env, ok ? (double)total : -1.0, &r));
  return r;
}

static napi_value Version(napi_env env, napi_callback_info info) {
  napi_value r;
  (void)info;
  NAPI_OK(napi_create_string_utf8(env, zs_version(), NAPI_AUTO_LENGTH, &r));
  return r;
}

static napi_value SelfTest(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], r;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  zs_ctx *ctx = ctx_for(env, argc ? arg_i32(env, argv[0], 0) : 0);
  if (!ctx) return NULL;
  uint64_t bad = 0;
  int rc = zs_selftest(ctx, &bad);
  if (rc != ZS_OK) return throw_code(env, rc, zs_last_error());
  NAPI_OK(napi_create_double(env, (double)bad, &r));
  return r;
}

static napi_value Init(napi_env env, napi_value exports) {
  napi_property_descriptor d[] = {
      {"compressBatch", NULL, CompressBatch, NULL, NULL, NULL, napi_default, NULL},
      {"decompressBatch", NULL, DecompressBatch, NULL, NULL, NULL, napi_default, NULL},
      {"deflateBound", NULL, DeflateBound, NULL, NULL, NULL, napi_default, NULL},
      {"bgzfOutLength", NULL, BgzfOutLength, NULL, NULL, NULL, napi_default, NULL},
      {"bgzfRangeOutLength", NULL, BgzfRangeOutLength, NULL, NULL, NULL, napi_default, NULL},
      {"version", NULL, Version, NULL, NULL, NULL, napi_default, NULL},
      {"selfTest", NULL, SelfTest, NULL, NULL, NULL, napi_default, NULL},
  };
  napi_define_properties(env, exports, sizeof d / sizeof d[0], d);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
