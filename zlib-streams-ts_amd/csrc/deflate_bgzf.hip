// deflate_bgzf.hip -- the layout and the frames of a BGZF batch (SAM specification 4.1).
//
// Each stream of such a batch is cut every B bytes into SEGMENTS (zs_plan_bgzf), each parsed and coded as
// a stream of its own and FINISHED: its last block carries BFINAL and is padded to a byte.  Every segment
// becomes a gzip member with the 18-byte BGZF header in front and crc32 + ISIZE behind; the stream ends
// with the 28-byte end-of-file block.  The layout runs per segment and joins them with the flushed
// layout's scan (deflate_flush.hip):
//   zs_k_bgzf_local   one thread per segment: its blocks' bit offsets relative to its own deflate data,
//                     BFINAL and bi_windup on the last one; the member's bytes (18 + data + 8), scanned
//                     within the workgroup; a member above 65,536 bytes fails its stream
//   zs_k_flush_tiles  the workgroups' sums, scanned
//   zs_k_bgzf_place   one thread per segment: the blocks rebased to the stream's output, the stream's
//                     length (+ 28) and status, the words zs_k_emit ORs into zeroed; a stream without
//                     segments is placed by the thread of its own index
//   zs_k_emit         unchanged, with the stream's out_off, absolute bit offsets and no wrapper
//   zs_k_bgzf_frame   after emit: every member's header and trailer and every stream's end-of-file block
// Who writes which byte of a word that a frame shares with deflate data: zs_k_bgzf_place zeroes the word,
// zs_k_emit ORs the data's bits into it (its zeroed-word + atomicOr rule for a block's first and last
// word), and zs_k_bgzf_frame, a later kernel on the same stream, stores the frame's bytes one by one --
// single-byte stores, which leave the neighbouring bytes as emit left them.
// Level 0 has no parse: zs_k_bgzf_stored writes frames, stored headers and pieces from host arithmetic.
#include "zs_kernels.h"
#include "zs_flush_scan.h"

// byte p < 18 of a member's header; bsize: the member's total size - 1
static __device__ __forceinline__ uint32_t zs_bgzf_header_byte(uint32_t p, uint32_t bsize) {
  // 1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 'B' 'C' 02 00 | BSIZE  (htslib bgzf_compress)
  constexpr uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0};
  return p < 16 ? h[p] : p == 16 ? (bsize & 0xffu) : (bsize >> 8) & 0xffu;
}
// byte p < 28 of the end-of-file block: the header with BSIZE 27, the empty static block 03 00, crc 0, ISIZE 0
static __device__ __forceinline__ uint32_t zs_bgzf_eof_byte(uint32_t p) {
  return p < ZS_BGZF_HEADER ? zs_bgzf_header_byte(p, ZS_BGZF_EOF - 1) : p == ZS_BGZF_HEADER ? 3u : 0u;
}

// segs: the segments' records (nblk as the parse left it); streams: the streams' records, zeroed but for
// `check`; pad collects "a member does not fit BSIZE" and "a stored block began before the slid window".
// segx[g], g <= M: the bytes of the members before g in g's workgroup; tile[w]: workgroup w's bytes.
__global__ __launch_bounds__(ZS_FLUSH_TILE) void zs_k_bgzf_local(const uint32_t* __restrict__ blk_base,
                                                                 zs_block* __restrict__ blocks,
                                                                 zs_stream* __restrict__ segs,
                                                                 const uint32_t* __restrict__ sstream,
                                                                 zs_stream* __restrict__ streams,
                                                                 uint64_t* __restrict__ segx,
                                                                 uint64_t* __restrict__ tile, uint32_t M) {
  __shared__ uint64_t tmp[4];
  const uint32_t g = blockIdx.x * ZS_FLUSH_TILE + threadIdx.x;
  uint64_t bytes = 0;
  if (g < M) {
    zs_block* blk = blocks + blk_base[g];
    // every piece is finished: Z_FINISH closes the pending block always, so a piece whose symbols end on the
    // 16,383-symbol cut keeps its trailing empty static block (the flushed layout's rule does not apply)
    const uint32_t nb = segs[g].nblk;
    uint64_t off = 0;
    uint32_t bad = 0;
    for (uint32_t b = 0; b < nb; b++) {
      zs_block k = blk[b];
      k.bit_off = off;
      if (k.type == 0) {
        if (k.last & 2u) bad = 1;
        off += 3;
        off = (off + 7) & ~7ull;
        off += 32 + 8ull * (k.in_end - k.in_start);
      } else {
        off += 3 + k.hdr_bits + k.data_bits;
      }
      k.bit_end = off;
      k.last = (k.last & 2u) | (b + 1 == nb ? 1u : 0u);
      if (k.last & 1u) off = (off + 7) & ~7ull;  // bi_windup (trees.ts:587-589)
      blk[b] = k;
    }
    segs[g].out_len = (uint32_t)(off >> 3);  // the deflate data's bytes
    bytes = ZS_BGZF_HEADER + (off >> 3) + ZS_BGZF_TRAILER;
    if (bytes > ZS_BGZF_MEMBER_MAX) bad = 1;  // never a wrapped BSIZE
    if (bad) atomicOr(&streams[sstream[g]].pad, 1u);
  }
  uint64_t total;
  const uint64_t pre = zs_flush_scan256(bytes, tmp, total);
  if (g <= M) segx[g] = pre;
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// The streams' out_off / out_cap here; every store lies in [out_off[s], out_off[s] + out_cap[s] rounded up
// to 4), and only when the stream fits.  A grid of max(M, n) threads: thread t places segment t and, if
// stream t has no segment, stream t.
__global__ __launch_bounds__(ZS_FLUSH_TILE) void zs_k_bgzf_place(const uint32_t* __restrict__ blk_base,
                                                                 zs_block* __restrict__ blocks,
                                                                 zs_stream* __restrict__ segs,
                                                                 const uint32_t* __restrict__ sfirst,
                                                                 const uint32_t* __restrict__ sstream,
                                                                 zs_stream* __restrict__ streams,
                                                                 const uint64_t* __restrict__ segx,
                                                                 const uint64_t* __restrict__ tile,
                                                                 const uint32_t* __restrict__ out_cap,
                                                                 uint8_t* __restrict__ out,
                                                                 const uint64_t* __restrict__ out_off, uint32_t M,
                                                                 uint32_t n) {
  const uint32_t t = blockIdx.x * ZS_FLUSH_TILE + threadIdx.x;
  if (t < n && sfirst[t] == sfirst[t + 1]) {  // an empty stream: the end-of-file block alone
    streams[t].nsym = 0;
    streams[t].nblk = 0;
    streams[t].total_bits = 0;
    streams[t].out_len = ZS_BGZF_EOF;
    streams[t].status = ZS_BGZF_EOF <= out_cap[t] ? ZS_Z_STREAM_END : ZS_Z_BUF_ERROR;
  }
  const uint32_t g = t;
  if (g >= M) return;
  const uint32_t s = sstream[g];
  const uint32_t g0 = sfirst[s], g1 = sfirst[s + 1];
  auto at = [&](uint32_t x) { return tile[x / ZS_FLUSH_TILE] + segx[x]; };  // the bytes of all members before x
  const uint64_t first = at(g0);
  const uint64_t base = at(g) - first + ZS_BGZF_HEADER;  // this segment's deflate data in the stream's output
  const uint64_t out_len = at(g1) - first + ZS_BGZF_EOF;
  const int32_t status = streams[s].pad ? ZS_Z_STREAM_ERROR : out_len <= out_cap[s] ? ZS_Z_STREAM_END : ZS_Z_BUF_ERROR;
  segs[g].status = status;  // (zs_k_emit and zs_k_bgzf_frame skip the segments of a stream that failed)
  segs[g].total_bits = 8 * base;
  if (g == g0) {  // (check stays: zs_k_copy_check's)
    streams[s].nsym = 0;
    streams[s].nblk = g1 - g0;
    streams[s].total_bits = 8 * (out_len - ZS_BGZF_EOF);
    streams[s].out_len = (uint32_t)out_len;
    streams[s].status = status;
  }
  if (status != ZS_Z_STREAM_END) return;
  // the blocks to the stream's output; the first and last word of each zeroed (zs_k_emit's atomic OR targets,
  // which the frame's bytes may share)
  uint32_t* ow = (uint32_t*)(out + out_off[s]);
  zs_block* blk = blocks + blk_base[g];
  const uint32_t nb = segs[g].nblk;
  for (uint32_t b = 0; b < nb; b++) {
    const uint64_t o0 = blk[b].bit_off + 8 * base, o1 = blk[b].bit_end + 8 * base;
    blk[b].bit_off = o0;
    blk[b].bit_end = o1;
    ow[o0 >> 5] = 0;
    ow[(o1 - 1) >> 5] = 0;
  }
}

// After zs_k_emit.  Thread t < M: segment t's header and trailer; thread M + s: stream s's end-of-file
// block.  seg_len: the segments' input lengths (ISIZE), seg_check their crc32.  Single-byte stores, all
// below the stream's out_len <= out_cap; a failed stream gets none.
__global__ __launch_bounds__(256) void zs_k_bgzf_frame(const zs_stream* __restrict__ segs,
                                                       const uint32_t* __restrict__ sstream,
                                                       const zs_stream* __restrict__ streams,
                                                       const uint32_t* __restrict__ seg_len,
                                                       const uint32_t* __restrict__ seg_check,
                                                       uint8_t* __restrict__ out,
                                                       const uint64_t* __restrict__ out_off, uint32_t M, uint32_t n) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t < M) {
    const zs_stream sg = segs[t];
    if (sg.status != ZS_Z_STREAM_END) return;
    uint8_t* o = out + out_off[sstream[t]];
    const uint64_t data = sg.total_bits >> 3;
    const uint32_t bsize = ZS_BGZF_HEADER + sg.out_len + ZS_BGZF_TRAILER - 1;
    for (uint32_t p = 0; p < ZS_BGZF_HEADER; p++) o[data - ZS_BGZF_HEADER + p] = (uint8_t)zs_bgzf_header_byte(p, bsize);
    const uint64_t tr = data + sg.out_len;
    const uint32_t crc = seg_check[t], isize = seg_len[t];
    for (uint32_t p = 0; p < 4; p++) {
      o[tr + p] = (uint8_t)(crc >> (8 * p));
      o[tr + 4 + p] = (uint8_t)(isize >> (8 * p));
    }
  } else if (t < M + n) {
    const zs_stream st = streams[t - M];
    if (st.status != ZS_Z_STREAM_END) return;
    uint8_t* o = out + out_off[t - M] + (st.out_len - ZS_BGZF_EOF);
    for (uint32_t p = 0; p < ZS_BGZF_EOF; p++) o[p] = (uint8_t)zs_bgzf_eof_byte(p);
  }
}

// ------------------------------------------------------------------- level 0
// One final stored block per piece: 01 | LEN | ~LEN | the piece (RFC 1951 3.2.4; htslib's level-0 branch).
// Member j of a stream of L bytes lies at j (B + 31); the stream is L + 31 ceil(L / B) + 28 bytes.  Row
// y < M of the grid is segment y: it writes the words whose first byte lies in its member, every byte of such
// a word mapped to a frame byte, a byte of the piece, or -- past the member's end -- the first bytes of what
// follows (the next member's header or the end-of-file block).  Row M + s is stream s: its results, and the
// words whose first byte lies in its end-of-file block.  So every word has one writer.
__global__ __launch_bounds__(256) void zs_k_bgzf_stored(const uint8_t* __restrict__ in,
                                                        const uint64_t* __restrict__ seg_in_off,
                                                        const uint32_t* __restrict__ seg_len,
                                                        const uint32_t* __restrict__ seg_check,
                                                        const uint32_t* __restrict__ sfirst,
                                                        const uint32_t* __restrict__ sstream,
                                                        const uint32_t* __restrict__ in_len, uint8_t* __restrict__ out,
                                                        const uint64_t* __restrict__ out_off,
                                                        const uint32_t* __restrict__ out_cap, uint32_t B, uint32_t M,
                                                        int32_t* __restrict__ status, uint32_t* __restrict__ out_len_res) {
  const uint32_t y = blockIdx.y;
  const uint32_t s = y < M ? sstream[y] : y - M;
  const uint64_t L = in_len[s];
  const uint64_t total = L + (uint64_t)(ZS_BGZF_HEADER + 5 + ZS_BGZF_TRAILER) * zs_bgzf_blocks(L, B) + ZS_BGZF_EOF;
  const bool fits = total <= out_cap[s];
  if (y >= M && blockIdx.x == 0 && threadIdx.x == 0) {
    status[s] = fits ? ZS_Z_STREAM_END : ZS_Z_BUF_ERROR;
    out_len_res[s] = fits ? (uint32_t)total : 0u;  // as zs_k_finish: failed streams produce nothing
  }
  if (!fits) return;
  uint32_t* ow = (uint32_t*)(out + out_off[s]);
  const uint64_t eof = total - ZS_BGZF_EOF;
  if (y >= M) {
    if (blockIdx.x) return;
    const uint64_t w = (eof + 3) / 4 + threadIdx.x;
    if (4 * w >= total) return;
    uint32_t word = 0;
    for (uint32_t j = 0; j < 4; j++)
      if (4 * w + j < total) word |= zs_bgzf_eof_byte((uint32_t)(4 * w + j - eof)) << (8 * j);
    ow[w] = word;
    return;
  }
  const uint32_t g = y, len = seg_len[g], crc = seg_check[g];
  const uint32_t member = ZS_BGZF_HEADER + 5 + len + ZS_BGZF_TRAILER;
  const uint64_t start = (uint64_t)(g - sfirst[s]) * (B + ZS_BGZF_HEADER + 5 + ZS_BGZF_TRAILER), end = start + member;
  const bool more = g + 1 < sfirst[s + 1];  // another member follows (a full one but perhaps the last)
  const uint32_t next_member = more ? ZS_BGZF_HEADER + 5 + seg_len[g + 1] + ZS_BGZF_TRAILER : ZS_BGZF_EOF;
  const uint8_t* src = in + seg_in_off[g];
  const uint64_t w_lo = (start + 3) / 4, w_hi = (end + 3) / 4;  // [w_lo, w_hi): first byte in [start, end)
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const uint64_t w = w_lo + ((uint64_t)blockIdx.x * 4 + q) * 256 + threadIdx.x;
    if (w >= w_hi) break;
    uint32_t word = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const uint64_t o = 4 * w + j;
      uint32_t b;
      if (o >= end) {  // (at most three bytes: the header of what follows)
        b = o >= total ? 0u : zs_bgzf_header_byte((uint32_t)(o - end), next_member - 1);
      } else {
        const uint32_t p = (uint32_t)(o - start);
        if (p < ZS_BGZF_HEADER) b = zs_bgzf_header_byte(p, member - 1);
        else if (p == ZS_BGZF_HEADER) b = 1u;  // BFINAL, BTYPE 00, then the byte's padding
        else if (p < ZS_BGZF_HEADER + 3) b = (len >> (8 * (p - ZS_BGZF_HEADER - 1))) & 0xffu;
        else if (p < ZS_BGZF_HEADER + 5) b = (~len >> (8 * (p - ZS_BGZF_HEADER - 3))) & 0xffu;
        else if (p < ZS_BGZF_HEADER + 5 + len) b = src[p - ZS_BGZF_HEADER - 5];
        else if (p < ZS_BGZF_HEADER + 9 + len) b = (crc >> (8 * (p - ZS_BGZF_HEADER - 5 - len))) & 0xffu;
        else b = (len >> (8 * (p - ZS_BGZF_HEADER - 9 - len))) & 0xffu;
      }
      word |= b << (8 * j);
    }
    ow[w] = word;
  }
}
