// inflate_bgzf.hip -- the members of BGZF files sized from their headers (the SAM specification,
// section 4.1).  zs_k_bgzf_size stands where zs_k_members_size stands in the members' search (inflate_members.hip):
// the same arguments, the same lane numbering, the same records.  A lane whose start has a header that can be
// trusted (zs_bgzf.h) writes {FINAL, start + BSIZE + 1, ISIZE, 0} from a handful of words; every other lane
// decodes as zs_k_members_size's does, under the same bound.  No atomics, no waits between workgroups, no
// barrier inside one.
#include "zs_kernels.h"
#include "zs_inflate.h"
#include "zs_bgzf.h"
#include "zs_cand.h"

// The kernel is shaped by the trusted lane: 256 starts to a workgroup, a start per thread, every thread's
// header checked at once (the words of its stream's and candidate's lookup, the header's words, the trailer's
// word: three dependent steps).  The decoding lane is the rare one -- a file's first plain member, a member
// with a name, a false candidate (1f 8b 08 04 comes up once in 2^32 offsets of compressed data).  A decoding
// lane needs 2,148 bytes of LDS for its Huffman state, so a wave owns ZS_BGZF_SLOTS states and its untrusted
// lanes take turns at them, SLOTS at a time in the order of their lane numbers; the round's count comes
// from a ballot and is the same in every lane, and a wave without an untrusted lane -- every wave of a BGZF
// file but the odd one -- leaves at the ballot and touches no LDS.  All starts untrusted (a plain gzip file
// given to this entry) is 16 rounds per wave: the LDS per decoding lane, which is what bounds the decoders of
// a CU, is zs_k_members_size's.
__global__ __launch_bounds__(ZS_BGZF_THREADS) void zs_k_bgzf_size(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len,
    const uint32_t* __restrict__ stile, uint32_t n, const uint64_t* __restrict__ tpre,
    const uint32_t* __restrict__ cand, uint64_t cap, uint32_t pass, zs_sync_rec* __restrict__ rec,
    uint8_t* __restrict__ trusted) {
  __shared__ zs_sync_tabs tabs[(ZS_BGZF_THREADS / 64u) * ZS_BGZF_SLOTS];
  const uint64_t x = (uint64_t)blockIdx.x * ZS_BGZF_THREADS + threadIdx.x;
  const uint64_t C = tpre[stile[n]];
  const bool live = C <= cap && x < n + C;
  zs_cand_lane l = {0u, ZS_CAND_FIRST, 0u};
  uint32_t s = 0, start = 0;
  bool decode = false;
  if (live) {
    l = zs_cand_lookup(x, n, stile, tpre);
    s = l.s;
    if (l.k != ZS_CAND_FIRST) start = cand[l.k];
    zs_sync_rec r = {ZS_SYNC_FINAL, 0u, 0u, 0u};
    const bool t = zs_bgzf_header(in + in_off[s], in_len[s], start, r.end, r.len);
    trusted[x] = t ? 1 : 0;
    if (t) rec[x] = r;
    decode = !t;
  }
  const unsigned long long m = __ballot(decode);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  const uint32_t rounds = ((uint32_t)__popcll(m) + ZS_BGZF_SLOTS - 1u) / ZS_BGZF_SLOTS;
  for (uint32_t round = 0; round < rounds; round++) {
    if (decode && rank / ZS_BGZF_SLOTS == round) {
      const uint32_t bound = zs_cand_bound(l, stile, tpre, cand, pass, in_len[s]);
      rec[x] = zs_members_size(in + in_off[s], in_len[s], start, bound, tabs[wv * ZS_BGZF_SLOTS + rank % ZS_BGZF_SLOTS]);
    }
  }
}
