// streams-api.mjs -- the batch entry the reference's src/streams-api.ts gains
// (SURVEY.md 8(b)): compressBatch / decompressBatch route whole batches of
// independent streams to the MI355X engine through the N-API addon.
//
// Per stream the result is exactly what piping that buffer alone through
//   new CompressionStream(format, {level})   (src/streams-api.ts -> src/mod/streams.ts:242-251)
//   new DecompressionStream(format)          (src/mod/streams.ts:253-262)
// yields when the whole buffer is written in ONE write() followed by close(),
// including the stream layer's error strings ("init failed: N",
// "process error: N", "finalization error: N", streams.ts:53,117,170).
// The CPU CompressionStream / DecompressionStream classes stay the
// reference's own; this module only adds the batch path.
import { createRequire } from "module";

const require = createRequire(import.meta.url);
const addon = require("./zsnapi.node");

// format -> windowBits exactly as streams.ts:220 (compression) and 233
// (decompression): loose comparisons, and every other value -- unknown strings,
// undefined -- falls through to 15 ("deflate", the zlib wrapper).
const compressWbits = (format) => (format == "gzip" ? 15 + 16 : format == "deflate-raw" ? -15 : 15);
const decompressWbits = (format) =>
  format == "gzip" ? 15 + 16 : format == "deflate-raw" ? -15 : format == "deflate64-raw" ? -16 : 15;
const Z_STREAM_END = 1;
const Z_STREAM_ERROR = -2;
const PHASE_INIT = 1, PHASE_FINISH = 3;

function streamError(status, phase) {
  if (phase === PHASE_INIT) return new Error(`init failed: ${status}`);
  if (phase === PHASE_FINISH) return new Error(`finalization error: ${status}`);
  return new Error(`process error: ${status}`);
}

function checkInputs(inputs) {
  if (!Array.isArray(inputs)) throw new TypeError("inputs must be an array of Uint8Array");
  return inputs.map((x) => {
    if (x instanceof Uint8Array) return x;
    if (ArrayBuffer.isView(x)) return new Uint8Array(x.buffer, x.byteOffset, x.byteLength);
    if (x instanceof ArrayBuffer) return new Uint8Array(x);
    throw new TypeError("inputs must be Uint8Array / ArrayBufferView / ArrayBuffer");
  });
}

// The device set of a batch (SURVEY.md 8(b) "device mask"): options.devices
// (an array of GPU indices: the batch is split into contiguous stream ranges,
// one per GPU, zs_pool) or options.device (one index); default GPU 0.
function devicesOf(options) {
  if (Array.isArray(options.devices)) return options.devices;
  return options.device === undefined ? 0 : options.device;
}

// options.dictionary: a preset dictionary.  The decompress entries use it as the z_stream
// driver would pass it to inflateSetDictionary (inflate.ts:1220-1249) -- for "deflate-raw"
// before the first inflate(), for "deflate" when inflate() returns Z_NEED_DICT; the compress
// entries as deflateSetDictionary right after deflateInit2_ (deflate.ts:367-424; "deflate-raw"
// and "deflate", levels 1..9: "gzip" or level 0 with one fail with "init failed: -2").  One
// ArrayBufferView shared by all inputs, or an array with one per input (null = none).
// Returns what the addon takes: undefined, or one Uint8Array | null per input.
function dictionariesOf(options, n) {
  const d = options.dictionary;
  if (d === undefined || d === null) return undefined;
  const view = (x) => {
    if (x instanceof Uint8Array) return x;
    if (ArrayBuffer.isView(x)) return new Uint8Array(x.buffer, x.byteOffset, x.byteLength);
    throw new TypeError("dictionary must be an ArrayBufferView, or an array of ArrayBufferView | null, one per input");
  };
  if (Array.isArray(d)) {
    if (d.length !== n) throw new TypeError("dictionary must be an ArrayBufferView, or an array with one entry per input");
    return d.map((x) => (x === null || x === undefined ? null : view(x)));
  }
  const shared = view(d);
  return new Array(n).fill(shared);
}

// options.strategy: deflateInit2_'s strategy (deflate.ts:289-290, :923-931), 0 Z_DEFAULT_STRATEGY ..
// 4 Z_FIXED.  A strategy that is not a number means 0 (the rule of `level`, streams.ts:221); a
// number out of range fails with "init failed: -2"; together with a dictionary it is a TypeError
// (no dictionaries with a strategy: zs_gpu.h).
export const Z_DEFAULT_STRATEGY = 0, Z_FILTERED = 1, Z_HUFFMAN_ONLY = 2, Z_RLE = 3, Z_FIXED = 4;
function strategyOf(options) {
  const s = typeof options.strategy == "number" ? options.strategy : 0;
  if (s !== 0 && options.dictionary !== undefined && options.dictionary !== null)
    throw new TypeError("strategy and dictionary cannot be combined");
  return s;
}

// options.windowBits (8..15) and options.memLevel (1..9): deflateInit2_'s windowBits and memLevel
// (deflate.ts:253-343).  A value that is not a number means the default, 15 and 8 (the rule of
// `level`, streams.ts:221); a number out of range -- and 8 for "deflate-raw" or "gzip" -- fails with
// "init failed: -2" (deflate.ts:281-294); values other than 15 / 8 together with a dictionary or a
// strategy are a TypeError (not built: zs_gpu.h).  Returns [deflateInit2_'s windowBits argument, memLevel].
function paramsOf(options, format) {
  const wb = typeof options.windowBits == "number" ? options.windowBits : 15;
  const ml = typeof options.memLevel == "number" ? options.memLevel : 8;
  if (!Number.isInteger(wb) || wb < 8 || wb > 15 || !Number.isInteger(ml) || ml < 1 || ml > 9 ||
      (wb === 8 && (format === "deflate-raw" || format === "gzip")))
    throw Object.assign(streamError(Z_STREAM_ERROR, PHASE_INIT), { code: String(Z_STREAM_ERROR) });
  if (wb !== 15 || ml !== 8) {
    if (options.dictionary !== undefined && options.dictionary !== null)
      throw new TypeError("windowBits / memLevel and dictionary cannot be combined");
    if (typeof options.strategy == "number" && options.strategy !== 0)
      throw new TypeError("windowBits / memLevel and strategy cannot be combined");
  }
  return [format === "deflate-raw" ? -wb : format === "gzip" ? wb + 16 : wb, ml];
}

// options.flushAt / options.flushEvery: Z_FULL_FLUSH points (deflate.ts:942-961; zs_deflate_batch_flush in
// zs_gpu.h).  flushAt: one array of positions for every input, or one array per input (null = none);
// flushEvery: N, the positions N, 2N, ... below each input's length.  Returns one array per input, or
// undefined without either.  Together with a dictionary, a strategy or windowBits / memLevel other than
// 15 / 8 they are a TypeError (not built); positions that do not increase or pass the input's length fail
// with "init failed: -2".
function flushOf(options, ins) {
  const at = options.flushAt, every = options.flushEvery;
  const has = (x) => x !== undefined && x !== null;
  if (!has(at) && !has(every)) return undefined;
  if (has(at) && has(every)) throw new TypeError("flushAt and flushEvery are alternatives");
  if (has(options.dictionary)) throw new TypeError("flush points and dictionary cannot be combined");
  if (typeof options.strategy == "number" && options.strategy !== 0)
    throw new TypeError("flush points and strategy cannot be combined");
  if ((typeof options.windowBits == "number" && options.windowBits !== 15) ||
      (typeof options.memLevel == "number" && options.memLevel !== 8))
    throw new TypeError("flush points and windowBits / memLevel cannot be combined");
  const pos = (x) => {
    if (!Number.isInteger(x) || x < 0 || x > 0xffffffff) throw new TypeError("flush positions are integers in 0 .. 2^32 - 1");
    return x;
  };
  if (has(every)) {
    if (!Number.isInteger(every) || every <= 0) throw new TypeError("flushEvery must be a positive integer");
    return ins.map((x) => {
      const out = [];
      for (let p = every; p < x.byteLength; p += every) out.push(p);
      return out;
    });
  }
  if (!Array.isArray(at)) throw new TypeError("flushAt must be an array of positions, or an array of such arrays, one per input");
  if (at.every((x) => typeof x == "number")) return ins.map(() => at.map(pos));
  if (at.length !== ins.length) throw new TypeError("flushAt must be an array of positions, or one array per input");
  return at.map((a) => {
    if (a === null || a === undefined) return [];
    if (!Array.isArray(a)) throw new TypeError("flushAt must be an array of positions, or one array per input");
    return a.map(pos);
  });
}

// options.bgzf: true, or the block's bytes 1 .. 65,280: every input becomes a BGZF file (SAM specification 4.1;
// zs_deflate_batch_bgzf in zs_gpu.h) -- blocks of that many input bytes (true: 65,280), each a gzip member with
// BSIZE, then the end-of-file block.  Returns block_bytes as the addon takes it (0 = 65,280), or undefined.
// Format "gzip" only; together with a dictionary, a strategy, windowBits / memLevel other than 15 / 8 or flush
// points a TypeError (not built); a block size out of range fails with "init failed: -2".
export const BGZF_BLOCK = 65280;
function bgzfOf(options, format) {
  const b = options.bgzf;
  if (b === undefined || b === null || b === false) return undefined;
  if (format !== "gzip") throw new TypeError('bgzf needs format "gzip"');
  const has = (x) => x !== undefined && x !== null;
  if (has(options.dictionary)) throw new TypeError("bgzf and dictionary cannot be combined");
  if (typeof options.strategy == "number" && options.strategy !== 0)
    throw new TypeError("bgzf and strategy cannot be combined");
  if ((typeof options.windowBits == "number" && options.windowBits !== 15) ||
      (typeof options.memLevel == "number" && options.memLevel !== 8))
    throw new TypeError("bgzf and windowBits / memLevel cannot be combined");
  if (has(options.flushAt) || has(options.flushEvery)) throw new TypeError("bgzf and flush points cannot be combined");
  if (b === true) return 0;
  if (!Number.isInteger(b) || b <= 0) throw new TypeError("bgzf is true or the block's bytes");
  return b;
}

// options.primed: true next to flushAt / flushEvery: no flush is written at the positions; the pieces between
// them are compressed in parallel, each primed with the 32 KiB in front of it (pigz's construction;
// zs_deflate_batch_primed in zs_gpu.h), and the output is one ordinary stream at nearly the single-stream
// ratio.  All three formats.  Without positions, or with bgzf, a TypeError; with a dictionary, a strategy or
// windowBits / memLevel it is refused as flush points are (flushOf).
function primedOf(options) {
  const p = options.primed;
  if (p === undefined || p === null || p === false) return false;
  if (p !== true) throw new TypeError("primed is true or false");
  const has = (x) => x !== undefined && x !== null;
  if (has(options.bgzf) && options.bgzf !== false) throw new TypeError("primed and bgzf cannot be combined");
  if (!has(options.flushAt) && !has(options.flushEvery)) throw new TypeError("primed needs flushAt or flushEvery");
  return true;
}

// The addon runs each batch on a worker thread (napi_async_work) and settles a
// Promise: the event loop is not blocked while the GPU works.
async function runCompress(inputs, format, options) {
  options = options || {};
  const [wbits, memLevel] = paramsOf(options, format);
  // streams.ts:221: a level that is not a number means Z_DEFAULT_COMPRESSION (-1 -> 6, deflate.ts:268-270)
  const level = typeof options.level == "number" ? options.level : -1;
  let res;
  try {
    const ins = checkInputs(inputs);
    const primed = primedOf(options);
    const bgzf = bgzfOf(options, format);
    res = await addon.compressBatch(ins, wbits, level, devicesOf(options), dictionariesOf(options, ins.length),
                                    strategyOf(options), memLevel, flushOf(options, ins), bgzf, primed);
  } catch (e) {
    // argument validation of deflateInit2_ (deflate.ts:281-294) surfaces as the stream layer's init error
    if (e.code === String(Z_STREAM_ERROR)) throw streamError(Z_STREAM_ERROR, PHASE_INIT);
    throw e;
  }
  return res.outputs.map((out, i) => (res.status[i] === Z_STREAM_END ? out : streamError(res.status[i], PHASE_FINISH)));
}

// The length of the wrapper's header in front of the deflate data (zs_wrapper_header_len in zs_gpu.h): 0
// for "deflate-raw", 2 for "deflate", for "gzip" 10 plus FEXTRA / FNAME / FCOMMENT / FHCRC -- or 0 when the
// magic, the method or a reserved flag is wrong or the header does not end inside the input.
export function wrapperHeaderLength(input, format = "gzip") {
  if (format === "deflate-raw" || format === "deflate64-raw") return 0;
  if (format !== "gzip") return 2;
  const p = input, n = input.length;
  if (n < 10 || p[0] !== 0x1f || p[1] !== 0x8b || p[2] !== 8 || (p[3] & 0xe0)) return 0;
  let at = 10;
  if (p[3] & 4) {
    if (at + 2 > n) return 0;
    at += 2 + p[at] + (p[at + 1] << 8);
    if (at > n) return 0;
  }
  for (const f of [8, 16])
    if (p[3] & f) {
      while (at < n && p[at]) at++;
      if (at >= n) return 0;
      at++;
    }
  if (p[3] & 2) at += 2;
  return at <= n ? at : 0;
}

// options.restartPoints: one array per input (null = none) of [inPos, outPos] pairs, the input's restart
// points WITHOUT its start -- inPos the offset of the first byte behind a Z_FULL_FLUSH marker, outPos the
// uncompressed bytes before it (zs_inflate_batch_restart in zs_gpu.h; inflateSync, inflate.ts:1267-1337).
// The segments decode in parallel, with zlib semantics.  Needs outCapacity; with a dictionary it is a
// TypeError (not built).  Returns, per input, the flat pairs with the start -- [header length, 0] -- first.
// restartPoints: "scan": the engine finds the points from the bytes (zs_inflate_batch_sync in zs_gpu.h), for
// a caller without an index; the same conditions, and the same result as with the true points.
// options.members: true: every member of multi-member gzip inputs is decoded and the outputs are concatenated
// (zs_inflate_batch_members in zs_gpu.h).  "gzip" only, needs outCapacity; with a dictionary or restartPoints
// it is a TypeError (not built).  options.members: "bgzf": the same, with BGZF blocks sized from their headers
// (zs_inflate_batch_bgzf in zs_gpu.h); without outCapacity the output is sized from the headers too (capacityOf).
function restartOf(options, ins, format) {
  const r = options.restartPoints;
  if (options.members) {
    const bgzf = options.members === "bgzf";
    if (typeof options.members === "string" && !bgzf) throw new TypeError("members must be true, false or \"bgzf\"");
    if (format !== "gzip") throw new TypeError("members are a gzip notion (format must be \"gzip\")");
    if (!bgzf && (options.outCapacity === undefined || options.outCapacity === null))
      throw new TypeError("members need outCapacity");
    if (options.dictionary !== undefined && options.dictionary !== null)
      throw new TypeError("members and dictionary cannot be combined");
    if (r !== undefined && r !== null) throw new TypeError("members and restartPoints cannot be combined");
    return bgzf ? "bgzf" : "members";
  }
  if (r === undefined || r === null) return undefined;
  if (options.dictionary !== undefined && options.dictionary !== null)
    throw new TypeError("restartPoints and dictionary cannot be combined");
  if (options.outCapacity === undefined || options.outCapacity === null)
    throw new TypeError("restartPoints need outCapacity");
  if (format === "deflate64-raw") throw new TypeError("deflate64-raw has no restart points");
  if (r === "scan") return r;
  if (!Array.isArray(r) || r.length !== ins.length)
    throw new TypeError("restartPoints must be an array with one entry per input");
  const u32 = (x) => Number.isInteger(x) && x >= 0 && x <= 0xffffffff;
  return r.map((ps, i) => {
    if (ps === null || ps === undefined) ps = [];
    if (!Array.isArray(ps)) throw new TypeError("restartPoints: an array of [inPos, outPos] pairs, or null, per input");
    const flat = [wrapperHeaderLength(ins[i], format), 0];
    for (const pt of ps) {
      if (!Array.isArray(pt) || pt.length !== 2 || !u32(pt[0]) || !u32(pt[1]))
        throw new TypeError("restartPoints: [inPos, outPos] pairs of integers in 0 .. 2^32 - 1");
      flat.push(pt[0], pt[1]);
    }
    return flat;
  });
}

// options.ranges with members: "bgzf": [[vb, ve], ...], one pair of BigInt virtual offsets (coffset << 16n |
// uoffset) per input: the input's bytes between the two (zs_inflate_batch_bgzf_range in zs_gpu.h).  Many ranges
// over one file: pass the same Uint8Array once per range; it is copied once.  Without members: "bgzf" a TypeError.
function rangesOf(options, ins) {
  const r = options.ranges;
  if (r === undefined || r === null) return undefined;
  if (options.members !== "bgzf") throw new TypeError('ranges need members: "bgzf"');
  if (!Array.isArray(r) || r.length !== ins.length) throw new TypeError("ranges must be an array with one [vb, ve] pair per input");
  return r.map((p) => {
    if (!Array.isArray(p) || p.length !== 2 || typeof p[0] !== "bigint" || typeof p[1] !== "bigint" || p[0] < 0n ||
        p[1] < 0n || p[0] >= 1n << 64n || p[1] >= 1n << 64n)
      throw new TypeError("ranges: [vb, ve] pairs of BigInt virtual offsets");
    return [p[0], p[1]];
  });
}

// The capacities of a decompress call: the caller's; for members: "bgzf" without them each input's bgzfOutLength
// (zs_bgzf_out_len: the sum of ISIZE over its blocks' headers) rounded up to 4 -- a TypeError naming the input that
// is not BGZF throughout; with ranges each range's bgzfRangeOutLength.
function capacityOf(options, ins, ranges) {
  const c = options.outCapacity;
  if (options.members !== "bgzf" || (c !== undefined && c !== null)) return c;
  if (ranges)
    return ins.map((x, i) => {
      const n = addon.bgzfRangeOutLength(x, ranges[i][0], ranges[i][1]);
      if (n < 0) throw new TypeError("input " + i + ": the virtual offsets do not follow a chain of BGZF blocks: give outCapacity");
      return (n + 3) - ((n + 3) % 4);
    });
  return ins.map((x, i) => {
    const n = addon.bgzfOutLength(x);
    if (n < 0) throw new TypeError("input " + i + " is not BGZF throughout: give outCapacity");
    return (n + 3) - ((n + 3) % 4);
  });
}

/** The bytes a BGZF file produces, read from its headers, or null when it is not BGZF throughout. */
export function bgzfOutLength(input) {
  const n = addon.bgzfOutLength(input);
  return n < 0 ? null : n;
}

/** The bytes the range between two BigInt virtual offsets delivers, read from the headers, or null where the
 * offsets do not follow a chain of BGZF blocks. */
export function bgzfRangeOutLength(input, vb, ve) {
  const n = addon.bgzfRangeOutLength(input, vb, ve);
  return n < 0 ? null : n;
}

/** A virtual offset from a block's start in the compressed file and a position in the block's data. */
export const virtualOffset = (coffset, uoffset = 0) => (BigInt(coffset) << 16n) | BigInt(uoffset);

async function runDecompress(inputs, format, options) {
  options = options || {};
  const wbits = decompressWbits(format);
  const ins = checkInputs(inputs);
  // no outCapacity: unbounded output, as DecompressionStream (streams.ts:46,132-182); a caller cap is a cap
  // (a dictionary for "gzip" / "deflate64-raw" rejects with code "-2": inflateSetDictionary's Z_STREAM_ERROR)
  let res;
  try {
    const restart = restartOf(options, ins, format);
    const ranges = rangesOf(options, ins);
    res = await addon.decompressBatch(ins, wbits, capacityOf(options, ins, ranges), devicesOf(options),
                                      dictionariesOf(options, ins.length), restart, ranges);
  } catch (e) {
    // points the entry refuses (zs_gpu.h): ZS_STREAM_ERROR, reported as the stream layer reports it
    if (options.restartPoints && e.code === String(Z_STREAM_ERROR))
      throw Object.assign(streamError(Z_STREAM_ERROR, PHASE_INIT), { code: e.code, zmsg: e.message });
    throw e;
  }
  return res.outputs.map((out, i) => {
    if (res.status[i] === Z_STREAM_END) return out;
    const err = streamError(res.status[i], res.phase[i]);
    err.zmsg = res.message[i];  // the z_stream msg (inflate.ts:397-1031, inffast.ts:108,197,210)
    return err;
  });
}

const settle = (xs) => xs.map((x) => (x instanceof Error ? { status: "rejected", reason: x } : { status: "fulfilled", value: x }));

/** Compress every input as an independent stream; rejects with the first stream's error. */
export async function compressBatch(inputs, format = "deflate", options = {}) {
  const out = await runCompress(inputs, format, options);
  const bad = out.find((x) => x instanceof Error);
  if (bad) throw bad;
  return out;
}

/** Decompress every input as an independent stream; rejects with the first stream's error. */
export async function decompressBatch(inputs, format = "deflate", options = {}) {
  const out = await runDecompress(inputs, format, options);
  const bad = out.find((x) => x instanceof Error);
  if (bad) throw bad;
  return out;
}

/** Per-stream outcomes, Promise.allSettled style. */
export async function compressBatchSettled(inputs, format = "deflate", options = {}) {
  return settle(await runCompress(inputs, format, options));
}

export async function decompressBatchSettled(inputs, format = "deflate", options = {}) {
  return settle(await runDecompress(inputs, format, options));
}

// (nFlush: the stream's Z_FULL_FLUSH points, or its points with `primed`, 12 bytes each: zs_deflate_bound_flush)
export const deflateBound = (length, format = "deflate", nFlush = 0) =>
  addon.deflateBound(length, compressWbits(format)) + 12 * nFlush;

/** Per-stream results with the check value (the reference's strm.adler after the
 * stream: adler32 / crc32 of the uncompressed bytes for "deflate" / "gzip"). */
export async function compressBatchDetailed(inputs, format = "deflate", options = {}) {
  options = options || {};
  const level = typeof options.level == "number" ? options.level : -1;
  const ins = checkInputs(inputs);
  const [wbits, memLevel] = paramsOf(options, format);
  const primed = primedOf(options);
  const bgzf = bgzfOf(options, format);
  return addon.compressBatch(ins, wbits, level, devicesOf(options), dictionariesOf(options, ins.length),
                             strategyOf(options), memLevel, flushOf(options, ins), bgzf, primed);
}

export async function decompressBatchDetailed(inputs, format = "deflate", options = {}) {
  options = options || {};
  const ins = checkInputs(inputs);
  const restart = restartOf(options, ins, format);
  const ranges = rangesOf(options, ins);
  return addon.decompressBatch(ins, decompressWbits(format), capacityOf(options, ins, ranges), devicesOf(options),
                               dictionariesOf(options, ins.length), restart, ranges);
}
export const engineVersion = () => addon.version();
export const selfTest = (device = 0) => addon.selfTest(device);
