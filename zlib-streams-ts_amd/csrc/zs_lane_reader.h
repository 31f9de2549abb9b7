// zs_lane_reader.h -- one lane's bit reader over a member's input, shared by the
// lane-per-member kernel (inflate_lane.hip), the segmented walk and decode
// (inflate_seg.hip) and the restart-point search's size decode (zs_sync.h), the
// first and the last with the per-lane Huffman code of zs_lane_huff.h on top:
// clamped aligned words, one refill ahead, zero past the end.  Plain C++ but for
// the funnel shift, so the host stand-ins of tools/lane_host and tools/sync_host
// compile it too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct zs_lane_reader {
  const uint32_t* w4;  // the aligned words holding the member's bytes
  uint32_t sh, last;   // the member's offset in its first word; index of the word holding its last byte
  uint32_t n, pos;  // bytes moved into hold so far (a multiple of 4)
  uint64_t hold;
  uint32_t bits;
  uint32_t pf;      // input bytes [pos, pos + 4), loaded one refill ahead (zero past the end)
};

// the member: n > 0 bytes at src (an empty member's reader must not read its own
// address: the caller points w4 at a word it may read, with last = 0)
static __device__ __forceinline__ void zs_lr_init(zs_lane_reader& R, const uint8_t* src, uint32_t n) {
  R.n = n;
  R.sh = (uint32_t)((uintptr_t)src & 3u);
  R.w4 = reinterpret_cast<const uint32_t*>(src - R.sh);
  R.last = (R.sh + n - 1u) >> 2;
}
// input bytes [at, at + 4) (at a multiple of 4), zero past the end: two aligned
// word loads with clamped indices and a funnel shift -- no branch, so the load
// stays in flight until the refill that uses it (a branch per byte made the
// compiler wait on each byte in turn)
static __device__ __forceinline__ uint32_t zs_lr_load4(const zs_lane_reader& R, uint32_t at) {
  const uint32_t q = (at + R.sh) >> 2;
  const uint32_t lo = R.w4[min(q, R.last)], hi = R.w4[min(q + 1u, R.last)];
  const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, R.sh);
  const uint32_t valid = at < R.n ? R.n - at : 0u;
  return valid >= 4u ? v : v & ((1u << (8u * valid)) - 1u);
}
// bits < 32 -> bits >= 32: the prefetched word enters hold and the next one is
// requested, so its latency overlaps the decoding of the bits just added
static __device__ __forceinline__ void zs_lr_fill(zs_lane_reader& R) {
  R.hold |= (uint64_t)R.pf << R.bits;
  R.bits += 32;
  R.pos += 4;
  R.pf = zs_lr_load4(R, R.pos);
}
static __device__ __forceinline__ void zs_lr_drop(zs_lane_reader& R, uint32_t k) {
  R.hold >>= k;
  R.bits -= k;
}
// (re)start at byte `at`, a multiple of 4, with nothing held
static __device__ __forceinline__ void zs_lr_rewind(zs_lane_reader& R, uint32_t at) {
  R.pos = at;
  R.hold = 0;
  R.bits = 0;
  R.pf = zs_lr_load4(R, at);
}
// (re)start at any bit (64-bit: the restart-point search seeks to any byte of a stream of up to 4 GiB)
static __device__ __forceinline__ void zs_lr_seek(zs_lane_reader& R, uint64_t bit) {
  zs_lr_rewind(R, (uint32_t)(bit >> 5) << 2);
  zs_lr_fill(R);
  zs_lr_drop(R, (uint32_t)bit & 31u);
}
// bits consumed so far
static __device__ __forceinline__ uint64_t zs_lr_bitpos(const zs_lane_reader& R) {
  return (uint64_t)R.pos * 8u - R.bits;
}
// ... in 32 bits, for members under 512 MB (the host sends no others where this is used)
static __device__ __forceinline__ uint32_t zs_lr_bitpos32(const zs_lane_reader& R) { return R.pos * 8u - R.bits; }
// consumed bits beyond the input: a truncated stream (the exact path reports it)
static __device__ __forceinline__ bool zs_lr_over(const zs_lane_reader& R) {
  return zs_lr_bitpos(R) > (uint64_t)R.n * 8u;
}
static __device__ __forceinline__ uint32_t zs_lr_take(zs_lane_reader& R, uint32_t k) {  // k <= 32
  if (R.bits < k) zs_lr_fill(R);
  const uint32_t v = (uint32_t)R.hold & (k == 32 ? 0xffffffffu : ((1u << k) - 1));
  zs_lr_drop(R, k);
  return v;
}
static __device__ __forceinline__ void zs_lr_align(zs_lane_reader& R) { zs_lr_drop(R, R.bits & 7u); }
