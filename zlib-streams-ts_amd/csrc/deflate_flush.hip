// deflate_flush.hip -- the layout of a batch with Z_FULL_FLUSH points.
//
// Each stream of such a batch is k + 1 SEGMENTS (zs_plan_flush): the pieces between its flush
// points, each parsed and coded as a stream of its own (the reference clears the hash and sets
// strstart = block_start = insert = 0 at a full flush with all input consumed, deflate.ts:942-955).
// zs_k_layout walks one stream's blocks in one thread; a stream of thousands of segments would
// make that the step's longest kernel, so the flushed layout runs per segment and joins them
// with a scan:
//   zs_k_flush_local  one thread per segment: its blocks' bit offsets relative to its own
//                     byte-aligned start; the marker -- an empty stored block, 00 00 FF FF behind
//                     three header bits and the byte padding -- behind every flushed piece; the
//                     segment's bytes, scanned within the workgroup
//   zs_k_flush_tiles  the workgroups' sums, scanned
//   zs_k_flush_place  one thread per segment: the blocks rebased to the stream's output, the
//                     stream's length and status, the shared words zeroed
// zs_k_emit then runs over the segments with the STREAM's out_off and absolute bit offsets: the
// seams fall on byte boundaries, not word boundaries, and its zeroed-word + atomicOr rule covers
// them as it covers the seams between blocks.
#include "zs_kernels.h"
#include "zs_flush_scan.h"

// segs: the segments' records (nblk as the parse left it); streams: the streams' records, zeroed
// but for `check`; pad collects "a stored block began before the slid window" (as zs_k_layout's bad).
// segx[g], g <= M: the bytes of the segments before g in g's workgroup; tile[w]: workgroup w's bytes.
__global__ __launch_bounds__(ZS_FLUSH_TILE) void zs_k_flush_local(const uint32_t* __restrict__ blk_base,
                                                                  zs_block* __restrict__ blocks,
                                                                  zs_stream* __restrict__ segs,
                                                                  const uint32_t* __restrict__ sfirst,
                                                                  const uint32_t* __restrict__ sstream,
                                                                  zs_stream* __restrict__ streams,
                                                                  uint64_t* __restrict__ segx,
                                                                  uint64_t* __restrict__ tile, uint32_t M) {
  __shared__ uint64_t tmp[4];
  const uint32_t g = blockIdx.x * ZS_FLUSH_TILE + threadIdx.x;
  uint64_t bytes = 0;
  if (g < M) {
    const uint32_t s = sstream[g];
    const bool fin = g + 1 == sfirst[s + 1];  // the piece Z_FINISH closes
    zs_block* blk = blocks + blk_base[g];
    uint32_t nb = segs[g].nblk;
    // at a flush the pending block is closed only if it holds symbols (deflate.ts:1343, 1441:
    // `if (s._sym_next) FLUSH_BLOCK(s, 0)`); Z_FINISH closes it always
    if (!fin && nb && blk[nb - 1].sym_count == 0) nb--;
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
      k.last = (k.last & 2u) | (fin && b + 1 == nb ? 1u : 0u);  // BFINAL: the block Z_FINISH closes alone
      if (k.last & 1u) off = (off + 7) & ~7ull;  // bi_windup (trees.ts:587-589)
      blk[b] = k;
    }
    if (!fin) {
      // _tr_stored_block(s, 0, 0, 0) (deflate.ts:942-946, trees.ts:449-464); the plan keeps a slot for it
      zs_block m;
      m.sym_start = 0; m.sym_count = 0; m.in_start = 0; m.in_end = 0;
      m.type = 0; m.hdr_bits = 0; m.data_bits = 0; m.last = 0; m.pad = 0;
      m.bit_off = off;
      off = ((off + 3 + 7) & ~7ull) + 32;
      m.bit_end = off;
      blk[nb++] = m;
    }
    segs[g].nblk = nb;
    bytes = off >> 3;  // (a multiple of 8 bits either way)
    if (bad) atomicOr(&streams[s].pad, 1u);
  }
  uint64_t total;
  const uint64_t pre = zs_flush_scan256(bytes, tmp, total);
  if (g <= M) segx[g] = pre;
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// exclusive scan of tile[0 .. T) in place, one workgroup of 256
__global__ __launch_bounds__(ZS_FLUSH_TILE) void zs_k_flush_tiles(uint64_t* __restrict__ tile, uint32_t T) {
  __shared__ uint64_t tmp[4];
  uint64_t carry = 0;
  for (uint32_t t0 = 0; t0 < T; t0 += ZS_FLUSH_TILE) {
    const uint32_t t = t0 + threadIdx.x;
    const uint64_t v = t < T ? tile[t] : 0;
    uint64_t total;
    const uint64_t pre = zs_flush_scan256(v, tmp, total);
    if (t < T) tile[t] = carry + pre;
    carry += total;
    __syncthreads();  // tmp is read before the next round rewrites it
  }
}

// The streams' out_off / out_cap here; every store lies in [out_off[s], out_off[s] + out_cap[s]
// rounded up to 4), and only when the stream fits
__global__ __launch_bounds__(ZS_FLUSH_TILE) void zs_k_flush_place(const uint32_t* __restrict__ blk_base,
                                                                  zs_block* __restrict__ blocks,
                                                                  zs_stream* __restrict__ segs,
                                                                  const uint32_t* __restrict__ sfirst,
                                                                  const uint32_t* __restrict__ sstream,
                                                                  zs_stream* __restrict__ streams,
                                                                  const uint64_t* __restrict__ segx,
                                                                  const uint64_t* __restrict__ tile,
                                                                  const uint32_t* __restrict__ out_cap,
                                                                  uint8_t* __restrict__ out,
                                                                  const uint64_t* __restrict__ out_off, int wrap,
                                                                  uint32_t M) {
  const uint32_t g = blockIdx.x * ZS_FLUSH_TILE + threadIdx.x;
  if (g >= M) return;
  const uint32_t s = sstream[g];
  const uint32_t g0 = sfirst[s], g1 = sfirst[s + 1];
  auto at = [&](uint32_t x) { return tile[x / ZS_FLUSH_TILE] + segx[x]; };  // the bytes of all segments before x
  const uint32_t hl = wrap == 1 ? 2u : wrap == 2 ? 10u : 0u;
  const uint32_t tl = wrap == 1 ? 4u : wrap == 2 ? 8u : 0u;
  const uint64_t first = at(g0);
  const uint64_t base = hl + (at(g) - first);    // this segment's first byte in the stream's output
  const uint64_t tb = hl + (at(g1) - first);     // the stream's bytes before the trailer
  const uint64_t out_len = tb + tl;
  const int32_t status = streams[s].pad ? ZS_Z_STREAM_ERROR : out_len <= out_cap[s] ? ZS_Z_STREAM_END : ZS_Z_BUF_ERROR;
  segs[g].status = status;  // (zs_k_emit skips the blocks of a stream that failed)
  if (g == g0) {            // (check stays: zs_k_copy_check's)
    streams[s].nsym = 0;
    streams[s].nblk = g1 - g0;
    streams[s].total_bits = 8 * tb;
    streams[s].out_len = (uint32_t)out_len;
    streams[s].status = status;
  }
  if (status != ZS_Z_STREAM_END) return;
  // the blocks to the stream's output; the words more than one writer touches zeroed (atomic OR targets)
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
  if (g == g0)
    for (uint32_t i = 0; i < (hl + 3) / 4; i++) ow[i] = 0;
  if (g + 1 == g1)
    for (uint64_t by = tb > 0 ? tb - 1 : 0; by < (out_len + 3) / 4 * 4; by += 4) ow[by >> 2] = 0;
}
