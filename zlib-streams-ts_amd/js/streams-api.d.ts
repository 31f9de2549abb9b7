// Types of the batch entry (streams-api.mjs) the reference's src/streams-api.ts gains.
// Formats are strings as in streams.ts:220,233: anything other than the names
// below falls through to "deflate" (windowBits 15), exactly as the reference.
export type CompressionFormat = "deflate" | "deflate-raw" | "gzip";
export type DecompressionFormat = CompressionFormat | "deflate64-raw";

export interface BatchOptions {
  /** One GPU index (default 0). */
  device?: number;
  /** GPU indices: the batch is split into contiguous stream ranges, one per GPU (zs_pool). */
  devices?: number[];
}
export interface CompressBatchOptions extends BatchOptions {
  /** 0..9, or -1 / any non-number for the default (6), as CompressionStream's {level} (streams.ts:221). */
  level?: number;
  /** A preset dictionary ("deflate-raw" and "deflate", levels 1..9), as passed to deflateSetDictionary
   * right after deflateInit2_: one view shared by all inputs, or one per input (null = none).  "deflate"
   * outputs carry FDICT and DICTID.  With "gzip", or with level 0, the call fails with "init failed: -2". */
  dictionary?: ArrayBufferView | (ArrayBufferView | null)[];
  /** deflateInit2_'s strategy (deflate.ts:289-290, :923-931): 0 Z_DEFAULT_STRATEGY (any non-number),
   * 1 Z_FILTERED, 2 Z_HUFFMAN_ONLY, 3 Z_RLE (the reference's, which finds no run: Z_HUFFMAN_ONLY's bytes),
   * 4 Z_FIXED.  A number out of range fails with "init failed: -2" (code "-2" from the detailed entry);
   * together with `dictionary` it is a TypeError. */
  strategy?: number;
  /** deflateInit2_'s windowBits (deflate.ts:253-343): 8..15, the window is 1 << windowBits bytes (8 runs as 9;
   * "deflate" outputs carry it in CINFO); any non-number means 15.  A number out of range, and 8 with
   * "deflate-raw" or "gzip", fails with "init failed: -2" (code "-2").  Other than 15 it is a TypeError together
   * with `dictionary` or a `strategy` other than 0, and level 0 fails with "init failed: -2". */
  windowBits?: number;
  /** deflateInit2_'s memLevel: 1..9, the hash has memLevel + 7 bits and a block closes after
   * (1 << (memLevel + 6)) - 1 symbols; any non-number means 8.  The rules of `windowBits` hold for it. */
  memLevel?: number;
  /** Z_FULL_FLUSH points (deflate.ts:942-961), levels 1..9: positions 0 <= p1 < p2 < ... <= the input's length, one
   * array for every input or one array per input (null = none).  At each one the pending block is closed, an empty
   * stored block (00 00 FF FF) is written and the history is dropped, so a decoder can restart behind it and the
   * pieces are compressed in parallel.  Positions out of order or past the length, and level 0, fail with "init
   * failed: -2" (code "-2"); together with `dictionary`, a `strategy` other than 0 or `windowBits` / `memLevel`
   * other than 15 / 8 it is a TypeError. */
  flushAt?: number[] | (number[] | null)[];
  /** flushAt at N, 2N, ... below each input's length. */
  flushEvery?: number;
  /** true next to `flushAt` / `flushEvery`: no flush is written at the positions.  The pieces between them are
   * compressed in parallel, each primed with the 32 KiB in front of it as a preset dictionary (pigz's
   * construction), and the output is one ordinary stream that any decoder reads, at nearly the single-stream
   * ratio; every piece but the last still ends with 00 00 FF FF on a byte boundary.  All three formats, levels
   * 1..9.  Without positions, or with `bgzf`, a TypeError; with `dictionary`, a `strategy` or `windowBits` /
   * `memLevel` other than 15 / 8 a TypeError, as for the positions. */
  primed?: boolean;
  /** BGZF (SAM specification 4.1), format "gzip" only, levels 0..9: every input becomes blocks of 65,280 input
   * bytes (true) or of this many (1 .. 65,280), each a gzip member with the BC subfield and BSIZE, then the 28-byte
   * end-of-file block -- what bgzip, samtools, tabix, gzip -d and {members: "bgzf"} read.  The blocks compress in
   * parallel.  A block size above 65,280 fails with "init failed: -2" (code "-2"); another format, or together
   * with `dictionary`, a `strategy` other than 0, `windowBits` / `memLevel` other than 15 / 8 or flush points, it
   * is a TypeError. */
  bgzf?: boolean | number;
}
export const BGZF_BLOCK: 65280;
export const Z_DEFAULT_STRATEGY: 0;
export const Z_FILTERED: 1;
export const Z_HUFFMAN_ONLY: 2;
export const Z_RLE: 3;
export const Z_FIXED: 4;
export interface DecompressBatchOptions extends BatchOptions {
  /** Output cap per stream (bytes), one number for all or one per input.  Default: none -- the
   * output is unbounded, as DecompressionStream's; a stream over a given cap rejects. */
  outCapacity?: number | number[];
  /** A preset dictionary ("deflate-raw" and "deflate"), as passed to inflateSetDictionary: one view
   * shared by all inputs, or one per input (null = none).  A "deflate" input with FDICT and the wrong
   * dictionary fails with "process error: -3", without one with "process error: 2". */
  dictionary?: ArrayBufferView | (ArrayBufferView | null)[];
  /** Restart points (inflateSync, inflate.ts:1267-1337): per input (null = none) the [inPos, outPos] pairs of its
   * Z_FULL_FLUSH markers, without its start -- inPos the offset in the input of the first byte behind a marker,
   * outPos the uncompressed bytes before it.  The segments between the points decode in parallel and come back
   * as one stream, with zlib semantics (the reference's window-wrap copy is not reproduced on this path).  A
   * stream whose points do not decode it fails with "process error: -3", zmsg "restart points do not decode
   * the stream"; points out of order, or past the input, fail with "init failed: -2" (code "-2").  Needs
   * `outCapacity`; without it, with `dictionary` or for "deflate64-raw" it is a TypeError.
   * "scan": the engine finds the points from the bytes (a batched syncsearch, inflate.ts:1267-1283) -- for a
   * seekable .gz of another writer, or a flushed stream whose index was lost.  The same conditions and the
   * same results; a stream without a full-flush marker decodes as one segment. */
  restartPoints?: ([number, number][] | null)[] | "scan";
  /** Multi-member gzip files (BGZF, WARC records, `cat a.gz b.gz`): decode EVERY member of each input and
   * concatenate the outputs, as `gzip -d` does, instead of the first member alone.  The members are found from
   * the bytes: behind a member's trailer another starts where 1f 8b 08 and a flag byte without a reserved bit
   * follow; anything else ends the stream and is ignored.  A member that is truncated or corrupt fails its
   * input.  "gzip" only, needs `outCapacity` (the total of an input's members); with another format, without
   * `outCapacity`, with `dictionary` or with `restartPoints` it is a TypeError.  The members' index
   * (zs_last_members) is not offered here: the batch entries run on the device pool.
   * "bgzf": the same for BGZF files (bgzip output, BAM, tabix-indexed VCF), with every block whose header can be
   * trusted sized from its BSIZE and ISIZE instead of a decode of its data (zs_inflate_batch_bgzf in zs_gpu.h).
   * Every input whose headers tell the truth decodes exactly as with `true`; a block whose ISIZE is too small fails
   * its input with zmsg "incorrect length check".  Without `outCapacity` each input's capacity is its
   * `bgzfOutLength`; an input that is not BGZF throughout is then a TypeError that names it. */
  members?: boolean | "bgzf";
  /** With `members: "bgzf"`: one `[vb, ve]` pair of BigInt virtual offsets (coffset << 16n | uoffset, as .bai / .tbi /
   * .csi indexes hold them) per input; the result is the input's bytes between the two (zs_inflate_batch_bgzf_range
   * in zs_gpu.h).  For many ranges over one file pass the same Uint8Array once per range: it is copied once.
   * Without `outCapacity` each range is sized from the headers (`bgzfRangeOutLength`).  Without `members: "bgzf"`
   * it is a TypeError. */
  ranges?: [bigint, bigint][];
}
/** The bytes a BGZF file produces, read from its headers (the sum of ISIZE over the blocks followed from offset 0),
 * or null when a member on the way is no BGZF block whose header can be trusted.  Host arithmetic, no GPU. */
export function bgzfOutLength(input: Uint8Array): number | null;
/** The bytes the range between two virtual offsets delivers, read from the headers; null where the offsets do not
 * follow a chain of BGZF blocks. */
export function bgzfRangeOutLength(input: Uint8Array, vb: bigint, ve: bigint): number | null;
/** coffset << 16n | uoffset */
export function virtualOffset(coffset: number | bigint, uoffset?: number | bigint): bigint;
/** The length of the wrapper's header in front of the deflate data: 0 for "deflate-raw", 2 for "deflate", for
 * "gzip" 10 plus FEXTRA / FNAME / FCOMMENT / FHCRC, or 0 when that header is malformed or does not fit. */
export function wrapperHeaderLength(input: Uint8Array, format?: string): number;
export type Settled<T> = { status: "fulfilled"; value: T } | { status: "rejected"; reason: Error & { zmsg?: string } };

export interface CompressDetail {
  status: Int32Array;
  /** strm.adler after each stream: adler32 ("deflate"), crc32 ("gzip") of the input, 1 for "deflate-raw". */
  check: Uint32Array;
  outputs: Uint8Array[];
}
export interface DecompressDetail extends CompressDetail {
  phase: Int32Array;
  message: string[];
  consumed: Int32Array;
}

export function compressBatch(inputs: ArrayBufferView[] | ArrayBuffer[], format?: string,
                              options?: CompressBatchOptions): Promise<Uint8Array[]>;
export function decompressBatch(inputs: ArrayBufferView[] | ArrayBuffer[], format?: string,
                                options?: DecompressBatchOptions): Promise<Uint8Array[]>;
export function compressBatchSettled(inputs: ArrayBufferView[] | ArrayBuffer[], format?: string,
                                     options?: CompressBatchOptions): Promise<Settled<Uint8Array>[]>;
export function decompressBatchSettled(inputs: ArrayBufferView[] | ArrayBuffer[], format?: string,
                                       options?: DecompressBatchOptions): Promise<Settled<Uint8Array>[]>;
export function compressBatchDetailed(inputs: ArrayBufferView[] | ArrayBuffer[], format?: string,
                                      options?: CompressBatchOptions): Promise<CompressDetail>;
export function decompressBatchDetailed(inputs: ArrayBufferView[] | ArrayBuffer[], format?: string,
                                        options?: DecompressBatchOptions): Promise<DecompressDetail>;
export function deflateBound(length: number, format?: string, nFlush?: number): number;
export function engineVersion(): string;
export function selfTest(device?: number): number;
