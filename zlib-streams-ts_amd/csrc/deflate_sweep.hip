// deflate_sweep.hip -- LZ77 match finding for deflate levels 4..9 on gfx950,
// streams of at most 65,537 bytes (the batch workloads' 64 KiB streams).
//
// What it computes is what zs_k_match (deflate_match.hip) computes: for EVERY
// position p, the (length, distance) the reference's longest_match
// (deflate.ts:1053-1115) returns at p for the full chain budget and for the
// budget >> 2 used when prev_length >= good_match (deflate.ts:1075-1077).  At
// levels 4..9 every position <= n-3 is inserted into its hash chain exactly
// once and in order, so p's chain is "every earlier inserted
// position with the same 15-bit hash, most recent first", cut at
// limit = p - MAX_DIST (deflate.ts:1060,1109) and by the budget.
//
// How is different.  Instead of following prev[] links (a dependent LDS
// round trip per chain step), the positions are counting-sorted by (hash,
// position) into a "member" array (zs_k_bucket).  Member k's chain is then
// simply members k-1, k-2, ... of its bucket, and the t-th predecessor is the
// t-th chain step.  zs_k_sweep gives each lane one member and sweeps t = 1,
// 2, ... for all 64 lanes at once: lane i reads the record of member
// k0 + i - t from a per-wave LDS ring (dense arrays: consecutive lanes read
// consecutive elements, conflict-free, and no load depends on the previous
// step), compares signatures with xor + ffbl, and keeps the first longest
// through a group maximum (sw_body below).
//
// Signatures: the 11 bytes after the hashed position's first byte, with a
// sentinel bit (SwSig<false>); for streams of 7-bit bytes (ASCII text) 8
// bytes [X, b3..b9] where X recovers the 9 bits of b0..b2 the 15-bit hash
// loses (SwSig<true>: bucket-mates with equal X and hash have equal b0..b2).
//
// Exactness (checked off the GPU by tools/emu/emu_bucket_sweep.c against a
// direct longest_match, and on the GPU by tests/test_gpu_deflate.py):
//   * liveness: record key = hash << 16 | pos; the head (t = 1) needs
//     key >= hash << 16 | max(limit, 1) (non-NIL, distance <= MAX_DIST,
//     deflate.ts:1376), the chain (t >= 2) key > hash << 16 | limit
//     (deflate.ts:1109); a member of another bucket fails both.  Liveness is
//     monotone in t.
//   * first strictly longer match wins (deflate.ts:1100-1105): the maximum of
//     a group's scores (matched bits, low bits = 7 - its place in the group)
//     is its first longest candidate; a group's winner replaces the best only
//     when longer.  Lengths are clamped to maxc = min(258, lookahead)
//     (deflate.ts:1068); the last positions of a stream re-walk exactly.
//   * a candidate whose whole signature matches is "long": the lanes holding
//     one extend it on the spot from the stream window (nice cut-off,
//     deflate.ts:1100-1105); long candidates beat every short one.
//   * both budgets in one sweep: the chain >> 2 result is a snapshot of the
//     state after step chain >> 2 (groups are cut there).
#include <hip/hip_runtime.h>
#include "zs_common.h"
#include "zs_kernels.h"
#include "zs_sweep_ring.h"
#include "zs_sweep_long.h"
#include "zs_sweep_ends.h"
#include <type_traits>
#include <utility>

// the window in LDS: ZS_SEG_WPOS inserted positions, a longest match past the
// last of them (258 bytes) and the 16-byte overreach of the word compares
#define ZS_SW_WIN_WORDS ((ZS_SEG_WPOS + 258u + 20u + 3u) / 4u + 2u)
#define ZS_SW_RING 128u  // records per wave (two blocks of 64 members), stored twice (mirror)
#define ZS_SW_MW 320u    // per-wave LDS window of member positions (chain + 64 <= ZS_SW_MW: level 7)
#ifndef ZS_SW_RUN_CAP
#define ZS_SW_RUN_CAP 16u  // chunks per run of the persistent ring at most (levels 4..6; 1, 4, 8, 16: DESIGN 4.2)
#endif

typedef __attribute__((address_space(3))) uint32_t zs_sw_lds_u32;
static __device__ __forceinline__ uint32_t sw_lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const zs_sw_lds_u32*)p;
}

static __device__ __forceinline__ uint32_t sw_hash(uint32_t w) {  // SURVEY A1, bytes 0..2 of w
  return (((w & 0xffu) << 10) ^ (((w >> 8) & 0xffu) << 5) ^ ((w >> 16) & 0xffu)) & ZS_HASH_MASK;
}

// -------------------------------------------------------------- zs_k_bucket
// One workgroup (4 waves) per stream: a counting sort of the inserted
// positions p <= n-3 by their hash, stable in position, into members[] (u16,
// the stream's range of the per-position workspace).  Pass 1 counts (32768 u16
// buckets, two per LDS word; all four waves), an exclusive scan turns the
// counts into offsets, and pass 2 -- one wave -- walks the positions in order,
// 64 per instruction, claiming slots with ONE ds_add_rtn_u32 per lane: gfx950
// applies same-address LDS atomics of one wave instruction in increasing lane
// order (zs_selftest checks it, including the 16-bit half form used here), so
// equal hashes get slots in position order; the other waves store the
// positions to their slots, a chunk's stores grouped by slot so that an
// instruction writes few lines.  Pass 1 hashes input words held
// in registers, pass 2 a 4 KiB LDS stage of the input.  Results of the
// positions that are not inserted (the last two) are zeroed.
#define ZS_BK_WPT (16384u / ZS_BK_THREADS)  // scan: count words per thread
#define ZS_BK_PPL (ZS_BK_THREADS / 64u)     // scan: partial sums per lane of the wave-level scan
#ifndef ZS_BK_PROF
#define ZS_BK_PROF 0  // timing experiments: wall-clock per pass summed over workgroups (0 in the product)
#endif
#if ZS_BK_PROF
__device__ unsigned long long zs_bk_stat[4];  // pass 1, scan, pass 2, workgroups
extern "C" int zs_bucket_stats(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(zs_bk_stat), sizeof(zs_bk_stat));
}
#define BK_MARK(i) do { if (threadIdx.x == 0) { const unsigned long long t_ = wall_clock64(); atomicAdd(&zs_bk_stat[i], t_ - bk_t); bk_t = t_; } } while (0)
#else
#define BK_MARK(i) do { } while (0)
#endif
#define ZS_BK_INFLIGHT 8  // pass 2: wave instructions (x 64 positions) per wait
#define ZS_BK_CHUNK 2048u  // pass 2: positions per chunk (input bytes staged in LDS, slots queued)
#define ZS_BK_KEYS 256u    // pass 2: a chunk's member stores are grouped by slot >> 8 (four 128-byte lines)
#define ZS_BK_HELPERS (ZS_BK_THREADS - 64u)                                    // pass 2: the threads of waves 1..7
#define ZS_BK_EPT ((ZS_BK_CHUNK + ZS_BK_HELPERS - 1u) / ZS_BK_HELPERS)  // ... and a chunk's queue entries per thread

// Workgroup barrier that waits for this wave's LDS operations only: the claim
// wave's loads of the next chunk and the helpers' member stores stay in flight.
static __device__ __forceinline__ void bk_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <bool ORD>  // false: claims ranked by zs_wave_match instead of the LDS atomics' lane order
__global__ __launch_bounds__(ZS_BK_THREADS) void zs_k_bucket(const uint8_t* __restrict__ in,
                                                            const uint64_t* __restrict__ in_off,
                                                            const uint32_t* __restrict__ in_len,
                                                            const uint64_t* __restrict__ pos_base,
                                                            const zs_sweep_seg* __restrict__ segs,
                                                            uint16_t* __restrict__ members, uint2* __restrict__ mres) {
  __shared__ uint32_t cnt[16384];
  // the scan's partial sums; in pass 2 its words are the key counters [0, KEYS) and the chunk's sorted order
  __shared__ uint32_t part[ZS_BK_KEYS + ZS_BK_CHUNK / 2];
  static_assert(ZS_BK_KEYS + ZS_BK_CHUNK / 2 >= ZS_BK_THREADS, "part[] holds the scan's partial sums");
  __shared__ uint32_t stg[ZS_BK_CHUNK / 4 + 2];
  __shared__ uint16_t q[2][ZS_BK_CHUNK];
  const zs_sweep_seg G = segs[blockIdx.x];
  const int s = (int)G.s;
  const uint32_t nrel = in_len[s] - G.base;  // bytes from the window's start to the stream's end
  const uint32_t tid = threadIdx.x;
  const uint8_t* src = in + in_off[s] + G.base;
  uint16_t* mem = members + G.mb;
  uint2* out = mres + pos_base[s] + G.base;
  // inserted positions of the window (deflate.ts:1367-1370: p <= n - 3), and the bytes their hashes read
  const uint32_t m = nrel > 2 ? min(nrel - 2, G.ohi) : 0u;
  const uint32_t n = min(nrel, m + 2u);
  if (nrel - m <= 2u)  // the window reaches the stream's end: its last positions are not inserted
    for (uint32_t p = m + tid; p < nrel; p += ZS_BK_THREADS) out[p] = make_uint2(0, 0);
  if (m == 0) return;
  for (uint32_t i = tid; i < 16384 / 4; i += ZS_BK_THREADS) reinterpret_cast<uint4*>(cnt)[i] = make_uint4(0, 0, 0, 0);
  const bool aligned = ((uintptr_t)src & 3u) == 0;
#if ZS_BK_PROF
  unsigned long long bk_t = wall_clock64();
  if (threadIdx.x == 0) atomicAdd(&zs_bk_stat[3], 1ull);
#endif
  __syncthreads();
  // pass 1: bucket sizes (unordered adds, all waves).  Thread t hashes the 16
  // positions [p0 + 16 t, +16) from 5 input words; the next 4 KiB block's words
  // are loaded before this block's adds (a load round trip per block, not per
  // four positions).
  {
    uint32_t w[5], nw[5];
    auto load5 = [&](uint32_t p0, uint32_t* x) __attribute__((always_inline)) {
#pragma unroll
      for (int k = 0; k < 5; k++) x[k] = zs_load_word(src, n, p0 + 16 * tid + 4 * k);
    };
    load5(0, nw);
    for (uint32_t p0 = 0; p0 < m; p0 += 16 * ZS_BK_THREADS) {
#pragma unroll
      for (int k = 0; k < 5; k++) w[k] = nw[k];
      if (p0 + 16 * ZS_BK_THREADS < m) load5(p0 + 16 * ZS_BK_THREADS, nw);
#pragma unroll
      for (uint32_t j = 0; j < 16; j++) {
        const uint32_t p = p0 + 16 * tid + j;
        const uint32_t h = sw_hash(__builtin_amdgcn_alignbyte(w[(j >> 2) + 1], w[j >> 2], j & 3u));
        if (p < m) atomicAdd(&cnt[h >> 1], 1u << (16u * (h & 1u)));
      }
    }
  }
  __syncthreads();
  BK_MARK(0);
  // exclusive scan: thread i owns words [WPT i, WPT i + WPT) (buckets 2 WPT i ...)
  {
    uint32_t sum = 0;
    for (uint32_t j = 0; j < ZS_BK_WPT; j++) {
      const uint32_t w = cnt[ZS_BK_WPT * tid + ((j + tid) & (ZS_BK_WPT - 1u))];  // rotated: threads hit different banks
      sum += (w & 0xffffu) + (w >> 16);
    }
    part[tid] = sum;
    __syncthreads();
    if (tid < 64) {  // scan of the partial sums, one wave
      uint32_t v[ZS_BK_PPL], t = 0;
#pragma unroll
      for (uint32_t j = 0; j < ZS_BK_PPL; j++) { v[j] = part[ZS_BK_PPL * tid + j]; t += v[j]; }
      uint32_t x = t;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (tid >= (uint32_t)d) x += y;
      }
      uint32_t run = x - t;
#pragma unroll
      for (uint32_t j = 0; j < ZS_BK_PPL; j++) { part[ZS_BK_PPL * tid + j] = run; run += v[j]; }
    }
    __syncthreads();
    uint32_t run = part[tid];
    for (uint32_t j = 0; j < ZS_BK_WPT; j++) {
      const uint32_t w = cnt[ZS_BK_WPT * tid + j];
      const uint32_t lo = w & 0xffffu;
      cnt[ZS_BK_WPT * tid + j] = run | ((run + lo) << 16);
      run += lo + (w >> 16);
    }
  }
  __syncthreads();
  BK_MARK(1);
  // pass 2: wave 0 claims the slots in position order, ZS_BK_CHUNK positions
  // at a time, into an LDS queue (slot of chunk position o at q[c & 1][o]);
  // waves 1..7 store the previous chunk's positions to their slots while it
  // claims the next one.  The member stores bound this pass by their number,
  // one write request per 128-byte line an instruction touches (a request per
  // member when stored in position order), so the helpers first group the
  // chunk's entries by slot >> 8 -- a counting sort of the queue indices over
  // ZS_BK_KEYS keys, in any order within a key -- and store them in that
  // order: neighbouring lanes then write neighbouring slots.  A chunk is PH
  // steps with a barrier each: the claim wave claims 64 ZS_BK_INFLIGHT
  // positions per step, the helpers count the keys, scan them (wave 1), place
  // the indices, store.  The input goes through LDS a chunk at a time (stg),
  // the next chunk's loads in flight in registers while this chunk's positions
  // are claimed, ZS_BK_INFLIGHT instructions per wait.
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  constexpr uint32_t PH = ZS_BK_CHUNK / (64 * ZS_BK_INFLIGHT);
  static_assert(PH == 4, "a chunk is four steps: count, scan, place, store");
  uint32_t* const kc = part;                                          // key counters, then the keys' next places
  uint16_t* const srt = reinterpret_cast<uint16_t*>(part + ZS_BK_KEYS);  // the chunk's queue indices grouped by key
  if (tid < ZS_BK_KEYS) kc[tid] = 0;
  uint32_t sl[ZS_BK_EPT];  // a helper's entries of the chunk: queue index ht + HELPERS k, its slot
  const uint32_t ht = tid - 64u;
  constexpr uint32_t CW = ZS_BK_CHUNK / 4 / 64;  // words per lane per chunk
  uint32_t nxt[CW + 1];
  auto fetch = [&](uint32_t c0) {
#pragma unroll
    for (uint32_t i = 0; i <= CW; i++) {
      const uint32_t w = 64 * i + lane;  // word index within the chunk (+ 2 words of overlap)
      const uint32_t at = c0 + 4 * w;
      uint32_t v = 0;
      if (w < ZS_BK_CHUNK / 4 + 2) {
        if (aligned && at + 4 <= n) v = *(const uint32_t*)(src + at);
        else
          for (uint32_t k = 0; k < 4; k++)
            if (at + k < n) v |= (uint32_t)src[at + k] << (8 * k);
      }
      nxt[i] = v;
    }
  };
  if (wave == 0) fetch(0);
  const uint32_t nch = (m + ZS_BK_CHUNK - 1) / ZS_BK_CHUNK;
  for (uint32_t c = 0; c <= nch; c++) {
    const uint32_t c0 = c * ZS_BK_CHUNK;
    const uint32_t c1 = min(m, c0 + ZS_BK_CHUNK);
    const uint32_t b0 = c0 - ZS_BK_CHUNK, cnt1 = min(m, c0) - b0;  // (helpers, c > 0: the previous chunk)
    const uint16_t* const qp = q[(c - 1) & 1u];
#pragma unroll
    for (uint32_t ph = 0; ph < PH; ph++) {
    const uint32_t g0 = c0 + 64 * ZS_BK_INFLIGHT * ph;
    if (wave == 0 && c < nch) {
      if (ph == 0) {
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (uint32_t i = 0; i <= CW; i++)
          if (64 * i + lane < ZS_BK_CHUNK / 4 + 2) stg[64 * i + lane] = nxt[i];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        if (c0 + ZS_BK_CHUNK < m) fetch(c0 + ZS_BK_CHUNK);
      }
      uint16_t* const qc = q[c & 1u];
      if (g0 < c1) {
        uint32_t a[ZS_BK_INFLIGHT], v[ZS_BK_INFLIGHT], sh[ZS_BK_INFLIGHT], e[ZS_BK_INFLIGHT], hh[ZS_BK_INFLIGHT];
#pragma unroll
        for (int j = 0; j < ZS_BK_INFLIGHT; j++) {
          const uint32_t p = g0 + 64 * j + lane;
          const uint32_t o = p - c0;
          const uint32_t h = sw_hash(__builtin_amdgcn_alignbyte(stg[(o >> 2) + 1], stg[o >> 2], o & 3u));
          hh[j] = h;
          sh[j] = 16u * (h & 1u);
          a[j] = sw_lds_addr(&cnt[h >> 1]);
          v[j] = p < c1 ? 1u << sh[j] : 0u;  // a lane past the chunk adds nothing
        }
        if (!ORD) {
          // order-independent: one add per distinct hash (its lowest lane), ranks by ballot
#pragma unroll
          for (int j = 0; j < ZS_BK_INFLIGHT; j++) {
            const uint32_t p = g0 + 64 * j + lane;
            const uint32_t h = hh[j];
            const uint64_t mm = zs_wave_match(h, p < c1);
            const uint32_t rank = (uint32_t)__builtin_popcountll(mm & ((1ull << lane) - 1ull));
            const uint32_t lead = mm ? (uint32_t)__builtin_ctzll(mm) : lane;
            uint32_t old = 0;
            if (p < c1 && lead == lane)
              old = atomicAdd(&cnt[h >> 1], (uint32_t)__builtin_popcountll(mm) << sh[j]);
            old = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(lead * 4u), (int)old);
            e[j] = old + (rank << sh[j]);
          }
        } else {
        // in order: instruction j's adds land after instruction j-1's (LDS executes a wave's ops in order)
        asm volatile(
            "ds_add_rtn_u32 %0, %8, %16\n\t"
            "ds_add_rtn_u32 %1, %9, %17\n\t"
            "ds_add_rtn_u32 %2, %10, %18\n\t"
            "ds_add_rtn_u32 %3, %11, %19\n\t"
            "ds_add_rtn_u32 %4, %12, %20\n\t"
            "ds_add_rtn_u32 %5, %13, %21\n\t"
            "ds_add_rtn_u32 %6, %14, %22\n\t"
            "ds_add_rtn_u32 %7, %15, %23\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(e[0]), "=&v"(e[1]), "=&v"(e[2]), "=&v"(e[3]), "=&v"(e[4]), "=&v"(e[5]), "=&v"(e[6]), "=&v"(e[7])
            : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(v[0]),
              "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7])
            : "memory");
        }
#pragma unroll
        for (int j = 0; j < ZS_BK_INFLIGHT; j++) {
          const uint32_t p = g0 + 64 * j + lane;
          if (p < c1) qc[p - c0] = (uint16_t)(e[j] >> sh[j]);
        }
      }
    } else if (wave != 0 && c > 0) {
      if (ph == 0) {  // the keys' counts
#pragma unroll
        for (uint32_t k = 0; k < ZS_BK_EPT; k++) {
          const uint32_t o = ht + ZS_BK_HELPERS * k;
          sl[k] = o < cnt1 ? (uint32_t)qp[o] : 0u;
          if (o < cnt1) atomicAdd(&kc[sl[k] >> 8], 1u);
        }
      } else if (ph == 1) {  // exclusive scan of the counts: the keys' first places (one wave)
        if (wave == 1) {
          constexpr uint32_t KPL = ZS_BK_KEYS / 64u;
          uint32_t v[KPL], t = 0;
#pragma unroll
          for (uint32_t j = 0; j < KPL; j++) { v[j] = kc[KPL * lane + j]; t += v[j]; }
          uint32_t x = t;
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= (uint32_t)d) x += y;
          }
          uint32_t run = x - t;
#pragma unroll
          for (uint32_t j = 0; j < KPL; j++) { kc[KPL * lane + j] = run; run += v[j]; }
        }
      } else if (ph == 2) {  // places: any order within a key
#pragma unroll
        for (uint32_t k = 0; k < ZS_BK_EPT; k++) {
          const uint32_t o = ht + ZS_BK_HELPERS * k;
          if (o < cnt1) srt[atomicAdd(&kc[sl[k] >> 8], 1u)] = (uint16_t)o;
        }
      } else {  // the stores, and the counters cleared for the next chunk
        for (uint32_t i = ht; i < cnt1; i += ZS_BK_HELPERS) {
          const uint32_t o = srt[i];
          mem[qp[o]] = (uint16_t)(b0 + o);
        }
        if (ht < ZS_BK_KEYS) kc[ht] = 0;
      }
    }
    bk_lds_barrier();
    }
  }
  BK_MARK(2);
}
template __global__ void zs_k_bucket<true>(const uint8_t*, const uint64_t*, const uint32_t*, const uint64_t*,
                                           const zs_sweep_seg*, uint16_t*, uint2*);
template __global__ void zs_k_bucket<false>(const uint8_t*, const uint64_t*, const uint32_t*, const uint64_t*,
                                            const zs_sweep_seg*, uint16_t*, uint2*);

// --------------------------------------------------------------- zs_k_sweep
static __device__ __forceinline__ uint32_t sw_word(const uint32_t* win, uint32_t off) {
  const uint32_t i = off >> 2;
  return __builtin_amdgcn_alignbyte(win[i + 1], win[i], off & 3u);
}

// exact length of a candidate whose first `from` bytes match, clamped to maxc
static __device__ __forceinline__ uint32_t sw_extend(const uint32_t* win, uint32_t p, uint32_t q, uint32_t maxc,
                                                     uint32_t from) {
  uint32_t k = from;
  while (k < maxc) {
    const uint32_t y = sw_word(win, q + k) ^ sw_word(win, p + k);
    if (y) { k += (uint32_t)(__builtin_ctz(y) >> 3); break; }
    k += 4;
  }
  return k < maxc ? k : maxc;
}

static __device__ __forceinline__ uint32_t max3(uint32_t a, uint32_t b, uint32_t c) {
  return max(max(a, b), c);  // one v_max3_u32
}

// Candidate signatures.  A chain step compares the lane's own signature with a
// candidate's and yields the index of the first differing bit (the "matched
// bits"); its byte is the signature's matched-byte count sigma.
//
// SwSig<false>, any stream: the 11 bytes [q, q + 11) in three words.  A
// record's third word keeps bytes 8..10 (byte 11 zeroed) and the lane's own
// third word carries a sentinel bit 24, so the xor of the third words always
// has bit 24 set and the count saturates at 88 (all 11 bytes) by itself.
// sigma is the match length (>= 3 within a bucket unless the hash collides).
//
// SwSig<true>, streams whose bytes are all < 0x80 (text): two words, 8 bytes
// [X, b3 .. b9].  Bytes 0..2 hash to the bucket; of their 24 bits
// the 15-bit hash loses 9 -- b0[5:7], and b1[0:2], b1[5:7] (which the hash
// only has xor-ed with b2[5:7] and b0[0:2]) -- and with bit 7 of every byte
// clear, the 7 bits X = b0[5:6] | b1[0:2] << 2 | b1[5:6] << 5 recover them: in
// one bucket, equal X <=> equal first three bytes.  So sigma = 0 means "not a
// match" (a hash collision) and sigma >= 1 means a match of sigma + 2 bytes;
// the count saturates at 64 (min3 with 64).  A step is six VALU instead of
// nine.
static __device__ __forceinline__ uint32_t sw_x7(uint32_t w) {
  const uint32_t b0 = w & 0xffu, b1 = (w >> 8) & 0xffu;
  return ((b0 >> 5) & 3u) | ((b1 & 7u) << 2) | (((b1 >> 5) & 3u) << 5);
}
template <bool A7>
struct SwSig;
template <>
struct SwSig<false> {
  static constexpr uint32_t LONG = 88u;  // all 11 bytes: the exact length needs the window
  static constexpr uint32_t THR0 = 23u;  // sigma 2 (B << 3 | 7): no match yet
  static constexpr uint32_t EXT = 11u;   // a long candidate's known bytes
  uint32_t a, b, c;  // the lane's own signature: its record's words, c with the sentinel (SwWave::start)
  static __device__ __forceinline__ uint4 rec(const uint32_t* win, uint32_t q, uint32_t w0) {
    return make_uint4(w0, sw_word(win, q + 4), sw_word(win, q + 8) & 0x00ffffffu, 0u);
  }
  __device__ __forceinline__ uint32_t mbits(uint32_t x, uint32_t y, uint32_t z) const {
    uint32_t f0, f1, f2;
    asm("v_ffbl_b32 %0, %1" : "=v"(f0) : "v"(x ^ a));
    asm("v_ffbl_b32 %0, %1\n\tv_add_u32_e64 %0, %0, 32 clamp" : "=&v"(f1) : "v"(y ^ b));
    asm("v_ffbl_b32 %0, %1\n\tv_add_u32_e32 %0, 64, %0" : "=&v"(f2) : "v"(z ^ c));
    // ffbl(0) = ~0 and the clamped add keep "no difference" at ~0; f2 <= 88 (the sentinel)
    return min(min(f0, f1), f2);
  }
  template <uint32_t U>
  __device__ __forceinline__ uint32_t step(uint32_t x, uint32_t y, uint32_t z) const {
    return (mbits(x, y, z) & ~7u) | (7u - U);  // one v_and_or_b32
  }
  template <uint32_t U>
  __device__ __forceinline__ uint32_t step(uint32_t x, uint32_t y, uint32_t z, uint64_t lm) const {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(step<U>(x, y, z)), "s"(lm));
    return r;
  }
  static __device__ __forceinline__ uint32_t len(uint32_t sigma) { return sigma; }
};
template <>
struct SwSig<true> {
  static constexpr uint32_t LONG = 64u;  // all 8 signature bytes: a match of >= 10 bytes
  static constexpr uint32_t THR0 = 7u;   // sigma 0
  static constexpr uint32_t EXT = 10u;
  uint32_t a, b;  // the lane's own signature: its record's words
  // (the record's third word: the four bytes past the signature, which a long
  // candidate's first extension step compares -- from the ring, not the window)
  static __device__ __forceinline__ uint4 rec(const uint32_t* win, uint32_t q, uint32_t w0) {
    return make_uint4(sw_x7(w0) | (sw_word(win, q + 3) << 8), sw_word(win, q + 6), sw_word(win, q + EXT), 0u);
  }
  __device__ __forceinline__ uint32_t mbits(uint32_t x, uint32_t y, uint32_t) const {
    uint32_t f0, f1;
    asm("v_ffbl_b32 %0, %1" : "=v"(f0) : "v"(x ^ a));
    asm("v_ffbl_b32 %0, %1\n\tv_add_u32_e64 %0, %0, 32 clamp" : "=&v"(f1) : "v"(y ^ b));
    return min(min(f0, f1), 64u);  // one v_min3_u32
  }
  // the whole step -- mbits(x, y, .) with its low three bits replaced by 7 - U, the step's score at
  // place U of its group (SwWave) -- as ONE asm block of the same seven VALU.  The
  // compiler cannot see into an asm block and assumes that it writes its results with a destination
  // select; gfx950 wants one wait state between such a write and a VALU that reads it (the dst_sel
  // forwarding hazard), so a plain instruction that consumes a block's result straight behind it gets
  // an s_nop 0 in front.  With the min3 and the and_or inside, a step's result is first read by the
  // group's max tree, after the other steps.
  // (the first word in place in its register, the second through a scratch register t that is an
  // output only -- its first write is the second instruction, behind the last read of a and x and
  // with the read of y and b, so t may share any input's register, and it takes y's where y dies
  // here.  With y tied in and out, the compiler copied the word of two records of every group into
  // a free register first: two v_mov per group.  A block that wrote a register of the block before
  // it would meet the hazard rule above.)
  template <uint32_t U>
  __device__ __forceinline__ uint32_t step(uint32_t x, uint32_t y, uint32_t) const {
    uint32_t t;
    asm("v_xor_b32_e32 %0, %0, %3\n\t"
        "v_xor_b32_e32 %1, %2, %4\n\t"
        "v_ffbl_b32 %0, %0\n\t"
        "v_ffbl_b32 %1, %1\n\t"
        "v_add_u32_e64 %1, %1, 32 clamp\n\t"
        "v_min3_u32 %0, %0, %1, 64\n\t"
        "v_and_or_b32 %0, %0, -8, %5"
        : "+v"(x), "=v"(t)
        : "v"(y), "v"(a), "v"(b), "n"(7u - U));
    return x;
  }
  // ... and 0 for a lane outside lm (the masked groups' select)
  template <uint32_t U>
  __device__ __forceinline__ uint32_t step(uint32_t x, uint32_t y, uint32_t, uint64_t lm) const {
    uint32_t t;
    asm("v_xor_b32_e32 %0, %0, %3\n\t"
        "v_xor_b32_e32 %1, %2, %4\n\t"
        "v_ffbl_b32 %0, %0\n\t"
        "v_ffbl_b32 %1, %1\n\t"
        "v_add_u32_e64 %1, %1, 32 clamp\n\t"
        "v_min3_u32 %0, %0, %1, 64\n\t"
        "v_and_or_b32 %0, %0, -8, %5\n\t"
        "v_cndmask_b32_e64 %0, 0, %0, %6"
        : "+v"(x), "=v"(t)
        : "v"(y), "v"(a), "v"(b), "n"(7u - U), "s"(lm));
    return x;
  }
  static __device__ __forceinline__ uint32_t len(uint32_t sigma) { return sigma ? sigma + 2u : 2u; }
};

// Per-wave ring of candidate records, as separate dense arrays so that the 64
// lanes of a step read 64 consecutive elements (conflict-free): signature words
// 0..1 (8 B), word 2 (the 11-byte form only) and the liveness key
// hash << 16 | q.  Member j's record lives in slot j mod 128 and again 128
// slots later, so that a block's 64 steps read slots base .. base + 63 without
// wrapping.  A chunk builds every block it reads; the members' positions are
// not kept past two blocks (level 7 keeps them in a window of its own, mw).
//
// Both layouts number the members in blocks of 64 (block b = members 64 b ..
// 64 b + 63, chunk c's own block is c) and provide
//   put(b, lane, r)   this lane's record r of block b (b wave-uniform),
//   base(c, s, lane)  for chunk c's steps (64 s, 64 s + 64] -- members of the
//                     blocks c - s - 1 and c - s: step t reads slot base - t.
struct SwRing {
  uint2 ab[2 * ZS_SW_RING];
  uint32_t c[2 * ZS_SW_RING];
  uint32_t key[2 * ZS_SW_RING];
  __device__ __forceinline__ void put(int b, uint32_t lane, uint4 r) {
    const uint32_t i = (uint32_t)(64 * b + (int)lane) & (ZS_SW_RING - 1);
    ab[i] = make_uint2(r.x, r.y);
    ab[i + ZS_SW_RING] = make_uint2(r.x, r.y);
    c[i] = r.z;  // (A7: the bytes past the signature)
    c[i + ZS_SW_RING] = r.z;
    key[i] = r.w;
    key[i + ZS_SW_RING] = r.w;
  }
  static __device__ __forceinline__ uint32_t base(int c, uint32_t s, uint32_t lane) {
    return ((uint32_t)(64 * (c - (int)s - 1) + (int)lane) & (ZS_SW_RING - 1)) + 64u * s + 64u;
  }
};
// The persistent ring of levels 4..6 (chain <= 128, zs_sweep_ring.h): three
// blocks of 64 members, block b at slots 64 (b mod 3), which a wave keeps
// across the consecutive chunks of a run -- a chunk builds its own block only,
// the blocks before it are the previous chunks' -- and slots 0..63 again at
// 192..255, so that the 64 steps of a block read upwards from one wave-uniform
// base without wrapping, as they do in SwRing.  The key array doubles as the
// window of member positions: pos(c, lane, t) is the position of member
// 64 c + lane - t for a step t of chunk c that was swept.
struct SwRingP {
  uint2 ab[ZS_SWR_SLOTS + ZS_SWR_MIRROR];
  uint32_t c[ZS_SWR_SLOTS + ZS_SWR_MIRROR];
  uint32_t key[ZS_SWR_SLOTS + ZS_SWR_MIRROR];
  __device__ __forceinline__ void put(int b, uint32_t lane, uint4 r) {
    const uint32_t i = zs_swr_block_slot(b) + lane;
    ab[i] = make_uint2(r.x, r.y);
    c[i] = r.z;
    key[i] = r.w;
    if (zs_swr_mirrored(b)) {  // a block at slot 0 is written twice (the mirror)
      ab[i + ZS_SWR_SLOTS] = make_uint2(r.x, r.y);
      c[i + ZS_SWR_SLOTS] = r.z;
      key[i + ZS_SWR_SLOTS] = r.w;
    }
  }
  static __device__ __forceinline__ uint32_t base(int c, uint32_t s, uint32_t lane) { return zs_swr_base(c, s) + lane; }
  __device__ __forceinline__ uint32_t pos(int c, uint32_t lane, uint32_t t) const {
    return key[zs_swr_member_slot(c, lane, t)] & 0xffffu;
  }
};

// The lock-step sweep of one stream (the workgroup), for signature form A7.
//
// For chain step t every lane compares its position with the t-th
// predecessor's signature.  A step's score is its matched bits with the low
// three bits (the bit within the first differing byte, which must not count)
// replaced by 7 - u, u = the step's place in its GROUP of steps (8, or 4 where
// a block end or the chain >> 2 snapshot cuts it): one v_and_or.  The group's
// maximum score is then its longest candidate and, among equally long ones,
// the earliest -- the first maximum of deflate.ts:1100-1105 -- and the lane
// keeps it when it is longer than its best so far (thr = B << 3 | 7 for a best
// of B signature bytes).  A step costs the compare and the v_and_or; the
// group's fold is max3s + a compare + three selects.
//
// A candidate whose whole signature matches is "long": its exact length needs
// the window.  Such candidates are rare; when a group holds one for any lane,
// those lanes extend it on the spot (the record's position is in the ring),
// keeping the first longest and stopping at the first nice match
// (deflate.ts:1100-1105).  Long candidates beat every short one.
//
// Liveness (deflate.ts:1109, 1376) is monotone in t, so a block of 64 steps in
// which every live lane's LAST step is live is live throughout for those lanes:
// such a block runs with the exec mask of the live lanes and no per-step test.
// A block in which some lane's chain ends runs the masked form (the step's
// ballot of `key > klim` ands into the live mask, a dead lane's score is 0).
#ifndef ZS_SW_PROF
#define ZS_SW_PROF 0  // instrumentation: counts of chunks, groups, long branches and wave steps (0 in the product)
#endif
#if ZS_SW_PROF
// chunks, fast groups, groups in which a chain ends, long branches, wave steps; of the ends groups those that read
// the winners' keys and those that fail validation (zs_sweep_ends.h); opening groups that fail it
__device__ unsigned long long zs_sw_stat[8];
#define SW_STAT(i, v) do { if ((threadIdx.x & 63u) == __builtin_ctzll(__builtin_amdgcn_read_exec())) atomicAdd(&zs_sw_stat[i], (unsigned long long)(v)); } while (0)
extern "C" int zs_sw_stats(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(zs_sw_stat), sizeof(zs_sw_stat));
}
#else
#define SW_STAT(i, v) do { } while (0)
#endif

// f(integral_constant<uint32_t, u>) for u = 0 .. N - 1: a group's steps, each with its place as a constant
template <class F, uint32_t... U>
static __device__ __forceinline__ void sw_each_(F&& f, std::integer_sequence<uint32_t, U...>) {
  (f(std::integral_constant<uint32_t, U>{}), ...);
}
template <uint32_t N, class F>
static __device__ __forceinline__ void sw_each(F&& f) {
  sw_each_(f, std::make_integer_sequence<uint32_t, N>{});
}
template <uint32_t N>  // the maximum of a group's N scores
static __device__ __forceinline__ uint32_t sw_gmax(const uint32_t* sc) {
  static_assert(N == 8 || N == 4 || N == 3 || N == 1, "group sizes");
  if constexpr (N == 8) return max(max3(sc[0], sc[1], sc[2]), max3(sc[3], sc[4], max3(sc[5], sc[6], sc[7])));
  else if constexpr (N == 4) return max3(sc[0], sc[1], max(sc[2], sc[3]));
  else if constexpr (N == 3) return max3(sc[0], sc[1], sc[2]);
  else return sc[0];
}

// One lane's state while its chunk is swept: its position, the limits of its
// walk, and its best candidates so far.
template <bool A7>
struct SwLane {
  SwSig<A7> S;           // the position's own signature
  uint32_t p;            // the position (0 past the members)
  bool own;              // ... is one of the window's own: it gets a result
  uint32_t maxc, nice;   // deflate.ts:1068, 1078-1080
  uint32_t khead, klim;  // liveness: the head needs key >= khead, a chain step key > klim
  uint32_t long_m;       // a score at or above it is a long candidate (a tail lane records none)
  uint32_t own_ext;      // the lane's bytes past a full signature
  // the best short candidate: its group's maximum score (matched bits, 7 - its place in the group) and the
  // group's first step (0: none) -- the step itself, bt + 7 - (thr & 7), is formed once at the end
  uint32_t thr, bt, thr_s, bt_s;
  // best long candidate: its length (capped at nice) as lthr = len << 3 | 7, its step
  uint32_t lthr, lbt, lthr_s, lbt_s;
  uint64_t alive_m;  // (wave-uniform) the lanes whose chain has not ended
  uint32_t head;     // bit 0: head candidate valid; 0x8000: at exactly MAX_DIST
  bool snapped;      // (wave-uniform) step chain >> 2 has been folded
  __device__ __forceinline__ bool tail() const { return maxc <= 12u; }  // exact re-walk after the sweep
  __device__ __forceinline__ void snap() {  // the chain >> 2 result (deflate.ts:1075-1077)
    thr_s = thr;
    bt_s = bt;
    lthr_s = lthr;
    lbt_s = lbt;
    snapped = true;
  }
};

// One wave's sweep of a window: what its chunks share, and the pieces of one
// chunk's work -- start (the lanes' state), build (the ring's blocks), sweep
// (the chain steps) and settle (the results).  sw_body drives them.
// PR: the persistent ring (chain <= ZS_SWR_MAX_CHAIN; MW is then unused).
// U8: the chain budget and its quarter are multiples of 8 (zs_sweep_uniform8,
// levels 5..9), so after the opening group of steps 1..8 every group is
// exactly eight steps and the chain >> 2 snapshot falls on a group's end: the
// walk (run8) needs no group bounds and no 4-step forms.
template <bool A7, bool MW, bool PR, bool U8>
struct SwWave {
  using Sig = SwSig<A7>;
  using Lane = SwLane<A7>;
  using Ring = std::conditional_t<PR, SwRingP, SwRing>;
  const uint32_t* win;
  Ring* R;
  uint16_t* mw;
  const uint16_t* mem;
  // n: bytes from the window's start to the stream's end; m: the window's members (inserted positions)
  uint32_t n, m, lane;
  // the steps swept: the full chain (a demand-driven variant that swept chain >> 2
  // steps and left the rest to the parse lost: DESIGN 4.2, tools/variants/r05_paths.patch)
  uint32_t budget, budget_s, nice_cfg;
  int cc;           // the chunk swept (wave-uniform); the lane's member is k()
  zs_swr_range vr;  // PR: the blocks the ring holds
  // MW: the members k0 - budget .. k0 + 63 of the current chunk are kept in a
  // per-wave LDS window as their records are built, so the distances after
  // the sweep read positions from LDS instead of HBM (chain + 64 <= ZS_SW_MW)
  int mw0;  // member index of mw[0] (k0 - budget)

  __device__ __forceinline__ int k() const { return 64 * cc + (int)lane; }
  __device__ __forceinline__ uint32_t fetch(int j) const { return j >= 0 && (uint32_t)j < m ? (uint32_t)mem[j] : 0u; }
  __device__ __forceinline__ uint4 make_rec(uint32_t q) const {
    const uint32_t w0 = sw_word(win, q);
    uint4 r = Sig::rec(win, q, w0);
    r.w = (sw_hash(w0) << 16) | q;
    return r;
  }
  // block blk from its members' positions q (0: no member; key 0 fails every liveness test)
  __device__ __forceinline__ void build_blk(int blk, uint32_t q) {
    const int j = 64 * blk + (int)lane;
    const bool in = j >= 0 && (uint32_t)j < m;
    if (MW && (uint32_t)(j - mw0) < ZS_SW_MW) mw[j - mw0] = (uint16_t)q;  // (block 1 back reaches below k0 - budget when budget < 64)
    R->put(blk, lane, in ? make_rec(q) : make_uint4(0, 0, 0, 0));
    if constexpr (PR) vr = zs_swr_extend(vr, blk);
  }
  // PR builds on demand: only a block the ring does not hold (a run's first chunk, or after a skipped one)
  __device__ __forceinline__ bool missing(int blk) const { return !PR || !zs_swr_has(vr, blk); }
  // the position of member k - t for a step t that was swept: its block is in the ring
  __device__ __forceinline__ uint32_t member(uint32_t t) const {
    if constexpr (PR) return R->pos(cc, lane, t);
    const int j = k() - (int)t;
    return MW ? (uint32_t)mw[j - mw0] : (uint32_t)mem[j];
  }

  // start: the state of the lane at position p before the first step; returns its record
  __device__ __forceinline__ uint4 start(Lane& L, uint32_t p, bool mem_ok, bool own) const {
    // the lane's record is built once, and its own signature, hash and the
    // bytes past the signature are taken from it
    const uint4 rown = mem_ok ? make_rec(p) : make_uint4(0, 0, 0, 0);
    L.S.a = rown.x;
    L.S.b = rown.y;
    if constexpr (!A7) L.S.c = rown.z | 0x01000000u;
    L.own_ext = A7 ? rown.z : sw_word(win, p + Sig::EXT);
    L.p = p;
    L.own = own;
    const uint32_t h = rown.w >> 16;
    const uint32_t look = n - p;
    L.maxc = look < ZS_MAX_MATCH ? look : ZS_MAX_MATCH;  // deflate.ts:1068
    L.nice = look < nice_cfg ? look : nice_cfg;          // deflate.ts:1078-1080
    L.long_m = L.tail() ? 0xffffu : Sig::LONG;
    const uint32_t limit = p > ZS_MAX_DIST ? p - ZS_MAX_DIST : 0u;  // deflate.ts:1060
    L.khead = (h << 16) | (limit > 1u ? limit : 1u);
    L.klim = (h << 16) | limit;
    L.thr = L.thr_s = Sig::THR0;
    L.bt = L.bt_s = 0;
    L.lthr = L.lthr_s = ZS_SWL_NONE;
    L.lbt = L.lbt_s = 0;
    L.alive_m = 0;
    L.head = 0;
    L.snapped = budget_s <= 1u;
    return rown;
  }

  // build: the ring's blocks for chunk cc -- its own (from the lanes' records)
  // and the one before it (positions qb where they were loaded ahead)
  __device__ __forceinline__ void build(uint4 rown, uint32_t p, uint32_t qb, bool have_qb) {
    mw0 = 64 * cc - (int)budget;
    if (MW) mw[k() - mw0] = (uint16_t)p;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    R->put(cc, lane, rown);
    if constexpr (PR) vr = zs_swr_push(vr, cc);
    if (missing(cc - 1)) build_blk(cc - 1, have_qb ? qb : fetch(k() - 64));
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }

  // A group's fold: the longest candidate if longer than the best so far.
  // Long candidates (a full signature match) are rare: when a group holds one
  // for any lane, those lanes compare the next four bytes of their first long
  // candidate (its position is in the ring); a candidate matching those too is
  // extended byte-wise (rarer still).  Which of a group's long candidates a
  // lane keeps is zs_sweep_long.h's rule: lengths are capped at nice -- the
  // first nice candidate ends the walk (deflate.ts:1103) and ties with every
  // later one, so it stays first.
  // (gm: the maximum of the group's cnt scores sc, 0 for a lane that takes
  // none; its steps are t0 .. t0 + cnt - 1, and step t0 + u's record is
  // element cnt - 1 - u of the group's part gc, gk of the ring's c and key)
  __device__ __forceinline__ void fold(Lane& L, uint32_t gm, uint32_t t0, const uint32_t* sc, uint32_t cnt,
                                       const uint32_t* gc, const uint32_t* gk) const {
    const bool up = gm > (L.thr | 7u);  // longer than the best so far
    L.thr = up ? gm : L.thr;
    L.bt = up ? t0 : L.bt;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(gm >= L.long_m) != 0, 0)) {
      SW_STAT(3, 1);
      // the score of the long candidate at place u (zs_sweep_long.h)
      auto lscore = [&](uint32_t u) -> uint32_t {
        // the next four bytes: A7 records carry them (c), else from the window
        const uint32_t ls = cnt - 1u - u;
        const uint32_t x = (A7 ? gc[ls] : sw_word(win, (gk[ls] & 0xffffu) + Sig::EXT)) ^ L.own_ext;
        const uint32_t len = x ? Sig::EXT + ((uint32_t)__builtin_ctz(x) >> 3)
                               : sw_extend(win, L.p, gk[ls] & 0xffffu, L.maxc, Sig::EXT + 4u);
        return zs_swl_score(len, L.maxc, L.nice, u);
      };
      const bool lg = gm >= L.long_m && zs_swl_open(L.lthr, L.nice);
      // The group's maximum names a lane's first long step; nearly always it is
      // the lane's only one in the group.  Whether some lane has a second one is
      // counted per lane from the scores packed four to a word (a score is below
      // 128, and score + 0x80 - LONG has bit 7 exactly when the step is long),
      // and only then do those lanes visit their other long steps one by one.
      // (a lane whose chain ended has gm 0, its steps' scores anything: lg)
      uint32_t w[2] = {0, 0};
#pragma unroll
      for (uint32_t u = 0; u < 8; u++)
        if (u < cnt) w[u >> 2] |= sc[u] << (8u * (u & 3u));
      constexpr uint32_t LB = (0x80u - Sig::LONG) * 0x01010101u;
      const uint32_t nl = (uint32_t)__builtin_popcount((w[0] + LB) & 0x80808080u) +
                          (uint32_t)__builtin_popcount((w[1] + LB) & 0x80808080u);
      const uint64_t twice = __builtin_amdgcn_ballot_w64(lg && nl > 1u);
      uint32_t gl = 0;
      const uint32_t u1 = zs_swl_first(gm);
      if (lg) gl = lscore(u1);
      if (__builtin_expect(twice != 0, 0)) {
        if ((twice >> lane) & 1u) {
          uint32_t lm = 0;
#pragma unroll
          for (uint32_t u = 0; u < 8; u++) lm |= (u < cnt && sc[u] >= L.long_m) ? 1u << u : 0u;
          lm &= ~(1u << u1);
          while (lm) {
            gl = zs_swl_join(gl, lscore((uint32_t)__builtin_ctz(lm)));
            lm &= lm - 1u;
          }
        }
      }
      zs_swl_fold(gl, t0, &L.lthr, &L.lbt);  // (gl 0: no change)
    }
  }

  // Steps t0 .. t0 + N - 1 as one group: step t reads slot base - t, one
  // address per ring array for the group (its lowest slot: at()), immediate
  // offsets inside.
  struct Grp {
    const uint2* A;
    const uint32_t *C, *K;
  };
  template <uint32_t N>
  __device__ __forceinline__ Grp at(uint32_t base, uint32_t t0) const {
    const uint32_t lo = base - (t0 + (N - 1u));
    return Grp{R->ab + lo, R->c + lo, R->key + lo};
  }
  // (A7: the group's part of c, from the address of its part of ab)
  __device__ __forceinline__ const uint32_t* c_of(const Grp& g) const {
    if constexpr (A7) return R->c + ((sw_lds_addr(g.A) - sw_lds_addr(R->ab)) >> 3);
    else return g.C;
  }
  // Unmasked, for a group in which every live lane is live throughout.
  // (every lane runs it -- no divergent region, whose join costs register moves --
  // and a lane whose chain has ended folds nothing: its maximum is selected to
  // 0 on the alive_m pair itself)
  template <uint32_t N>
  __device__ __forceinline__ void group_fast(Lane& L, const Grp& g, uint32_t t0) const {
    uint32_t sc[N];
    sw_each<N>([&](auto uc) __attribute__((always_inline)) {
      constexpr uint32_t u = decltype(uc)::value;
      const uint2 ab = g.A[N - 1u - u];
      sc[u] = L.S.template step<u>(ab.x, ab.y, A7 ? 0u : g.C[N - 1u - u]);
    });
    const uint32_t gm = __builtin_amdgcn_inverse_ballot_w64(L.alive_m) ? sw_gmax<N>(sc) : 0u;
    fold(L, gm, t0, sc, N, c_of(g), g.K);
  }
  // Masked, for a group in which a chain ends: liveness is monotone in t (keys
  // fall with the member index), so a step is live iff its own key is (and the
  // lane was live when the group began); a dead lane's score is 0.  Every load
  // is issued before the first is waited for.
  // HEAD: the group begins the walk.  The head candidate (t0 = 1,
  // deflate.ts:1376) has its own liveness rule, key >= khead, and it starts
  // alive_m; the chain steps after it are live while their keys are.
  template <uint32_t N, bool HEAD>
  __device__ __forceinline__ void group_masked(Lane& L, const Grp& g, uint32_t t0) const {
    uint32_t sc[N], key[N];
    uint2 ab[N];
#pragma unroll
    for (uint32_t u = 0; u < N; u++) {
      key[u] = g.K[N - 1u - u];
      ab[u] = g.A[N - 1u - u];
    }
    if constexpr (HEAD) {
      const bool a1 = L.own && key[0] >= L.khead;
      L.head = a1 ? 1u | ((L.p - (key[0] & 0xffffu)) == ZS_MAX_DIST ? 0x8000u : 0u) : 0u;
      L.alive_m = __builtin_amdgcn_ballot_w64(a1);
    }
    uint64_t lm = L.alive_m;  // the live lanes
    sw_each<N>([&](auto uc) __attribute__((always_inline)) {
      constexpr uint32_t u = decltype(uc)::value;
      // (asm results go through locals: an asm operand cannot name a captured variable)
      if (!HEAD || u) {
        uint64_t gt;
        const uint32_t ku = key[u], klim = L.klim;
        asm("v_cmp_gt_u32_e64 %0, %1, %2" : "=s"(gt) : "v"(ku), "v"(klim));
        lm = gt & L.alive_m;
      }
      sc[u] = L.S.template step<u>(ab[u].x, ab[u].y, A7 ? 0u : g.C[N - 1u - u], lm);
    });
    L.alive_m = lm;  // the lanes live at the group's last step (an SGPR pair: the asm's, and-ed with one)
    fold(L, sw_gmax<N>(sc), t0, sc, N, c_of(g), g.K);
  }

  // A group of eight in which some lane's chain ends, behind its max tree: gm
  // is the maximum of the UNMASKED scores sc (0 for a lane outside a0, the
  // lanes live when the group began), last the lanes live at its last step, K
  // the group's part of the ring's keys.  Returns the lanes that are not settled.
  // zs_sweep_ends.h has the rule: a lane with dead steps keeps gm when it
  // neither raises its best nor is long -- no key is read -- or when it is not
  // long and its winner's step is live: that key alone is read, and only when
  // some such lane would raise its best.  Otherwise the wave loads the eight
  // keys, zeroes the dead steps' scores (they are still in registers) and takes
  // the maximum again.
  // HEAD: the opening group, whose step 0 is live for every lane of a0.
  template <bool HEAD>
  __device__ __forceinline__ uint64_t ends(const Lane& L, const uint32_t* K, uint64_t a0, uint64_t last,
                                           uint32_t gm) const {
    const uint64_t part = a0 & ~last;  // the lanes with dead steps
    const uint64_t raise = __builtin_amdgcn_ballot_w64(zs_swe_raises(gm, L.thr)) & part;
    uint64_t bad = __builtin_amdgcn_ballot_w64(zs_swe_long(gm, L.long_m)) & part;
    if (raise) {
      SW_STAT(5, 1);
      const uint32_t wk = ((const zs_sw_lds_u32*)K)[zs_swe_winner_slot(gm)];
      bad |= raise & ~__builtin_amdgcn_ballot_w64(zs_swe_winner_live(gm, wk, L.klim, HEAD));
    }
    return bad;
  }
  // ... and the piece for a group that fails: the maximum of the masked scores
  template <bool HEAD>
  __device__ __forceinline__ uint32_t remask(const Lane& L, const uint32_t* K, uint64_t a0, uint32_t* sc) const {
    SW_STAT(HEAD ? 7 : 6, 1);
    uint32_t key[8];
#pragma unroll
    for (uint32_t u = HEAD ? 1u : 0u; u < 8; u++) key[u] = K[7u - u];
    sw_each<8>([&](auto uc) __attribute__((always_inline)) {
      constexpr uint32_t u = decltype(uc)::value;
      if (!HEAD || u) {
        // (asm results go through locals: an asm operand cannot name a captured variable)
        uint64_t gt;
        const uint32_t ku = key[u], klim = L.klim;
        asm("v_cmp_gt_u32_e64 %0, %1, %2" : "=s"(gt) : "v"(ku), "v"(klim));
        uint32_t v;
        const uint32_t su = sc[u];
        asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(v) : "v"(su), "s"(gt));
        sc[u] = v;
      }
    });
    return __builtin_amdgcn_inverse_ballot_w64(a0) ? sw_gmax<8>(sc) : 0u;
  }

  // U8: steps 1..8, the group that opens the walk, in the same way.  The head
  // candidate (step 1, deflate.ts:1376) has its own liveness rule,
  // key >= khead, and starts alive_m; the chain steps after it are live while
  // their keys are, so the lanes alive after the group are the head's with a
  // live step 8.
  __device__ __forceinline__ void open8(Lane& L, const Grp& g) const {
    const uint32_t k1 = g.K[7], k8 = g.K[0];
    uint32_t sc[8];
    sw_each<8>([&](auto uc) __attribute__((always_inline)) {
      constexpr uint32_t u = decltype(uc)::value;
      const uint2 ab = g.A[7u - u];
      sc[u] = L.S.template step<u>(ab.x, ab.y, A7 ? 0u : g.C[7u - u]);
    });
    const bool a1 = L.own && k1 >= L.khead;
    L.head = a1 ? 1u | ((L.p - (k1 & 0xffffu)) == ZS_MAX_DIST ? 0x8000u : 0u) : 0u;
    const uint64_t a0 = __builtin_amdgcn_ballot_w64(a1);
    const uint64_t last = __builtin_amdgcn_ballot_w64(k8 > L.klim) & a0;
    uint32_t gm = a1 ? sw_gmax<8>(sc) : 0u;
    uint64_t bad = 0;
    if (last != a0) bad = ends<true>(L, g.K, a0, last, gm);
    if (__builtin_expect(bad != 0, 0)) gm = remask<true>(L, g.K, a0, sc);
    L.alive_m = last;
    fold(L, gm, 1u, sc, 8u, c_of(g), g.K);
  }

  // Steps [ta, tb] of a block (ta = 1 mod 4, tb = 0 mod 4, wave-uniform) in
  // groups of 8 (4 where the range or the snapshot cuts them).  A group in
  // which every live lane is still live at its last step runs unmasked with
  // the exec mask of the live lanes; otherwise masked.
  __device__ __forceinline__ void run(Lane& L, uint32_t base, uint32_t ta, uint32_t tb) const {
    // the next group's last key is read with this group's records: the fast-or-masked test waits on no load
    auto last_of = [&](uint32_t t0) __attribute__((always_inline)) {
      uint32_t t1 = t0 + 7u <= tb ? t0 + 7u : t0 + 3u;
      if (t0 <= budget_s && t1 > budget_s) t1 = budget_s;
      return t1;
    };
    if (ta > tb) return;
    uint32_t t0 = ta, t1 = last_of(ta);
    uint32_t kl = R->key[base - t1];
    while (L.alive_m) {
      const uint64_t last_live = __builtin_amdgcn_ballot_w64(kl > L.klim) & L.alive_m;
      const uint32_t n0 = t1 + 1u, n1 = n0 <= tb ? last_of(n0) : t1;
      kl = R->key[base - n1];
      SW_STAT(last_live == L.alive_m ? 1 : 2, 1);
      SW_STAT(4, t1 - t0 + 1u);
      if (last_live == L.alive_m) {
        if (t1 - t0 == 7u) group_fast<8>(L, at<8>(base, t0), t0);
        else group_fast<4>(L, at<4>(base, t0), t0);
      } else {
        if (t1 - t0 == 7u) group_masked<8, false>(L, at<8>(base, t0), t0);
        else group_masked<4, false>(L, at<4>(base, t0), t0);
      }
      if (t1 == budget_s) L.snap();
      if (n0 > tb) break;
      t0 = n0;
      t1 = n1;
    }
  }

  // U8: steps [ta, te] (ta = 1 mod 8, te = 0 mod 8) in groups of exactly eight.
  // The groups' addresses run down the ring, one subtraction per array and
  // group, and the next group's last key is this group's at an immediate offset
  // (for the range's last group that is a slot below the range, inside the
  // ring's arrays or the array before them: read, never used).
  __device__ __forceinline__ void run8(Lane& L, uint32_t base, uint32_t ta, uint32_t te) const {
    // (one name for the mask from here on: the loops around this one carry it in several copies that the
    // compiler cannot tell are equal, and each copy would be an SGPR-pair move per group)
    asm("" : "+s"(L.alive_m));
    Grp g = at<8>(base, ta);
    // (the key address runs eight slots below its group: the look-ahead key at offset 0, the group's above it)
    const zs_sw_lds_u32* k8 = (const zs_sw_lds_u32*)(g.K - 8);
    uint32_t kl = g.K[0];
    if (!L.alive_m) return;
    uint32_t t0 = ta;
    do {
      const uint64_t last_live = __builtin_amdgcn_ballot_w64(kl > L.klim) & L.alive_m;
      kl = k8[0];
      g.K = (const uint32_t*)(k8 + 8);
      SW_STAT(last_live == L.alive_m ? 1 : 2, 1);
      SW_STAT(4, 8u);
      // The steps run unmasked, and a group in which a chain ends validates its maximum behind the
      // max tree (ends: zs_sweep_ends.h); only a group that fails loads the steps' keys and zeroes the
      // dead steps' scores, group_masked's liveness rule.  (One copy of the steps, the max tree and
      // the fold with a conditional piece between them -- not group_fast and group_masked joined:
      // the join of the two forms cost register moves and flag tests in both, and the long branch
      // stood twice.)
      const uint64_t a0 = L.alive_m;  // the lanes live when the group begins
      uint32_t sc[8];
      sw_each<8>([&](auto uc) __attribute__((always_inline)) {
        constexpr uint32_t u = decltype(uc)::value;
        const uint2 ab = g.A[7u - u];
        sc[u] = L.S.template step<u>(ab.x, ab.y, A7 ? 0u : g.C[7u - u]);
        // (the steps stay in the order of their records' loads, two to a load, and each pair waits for its own
        // load alone: left to itself the scheduler began with a record of the last load but one.  LDS reads
        // may cross the barrier (0x180), so the loads still go out ahead.)
        if (u & 1u) __builtin_amdgcn_sched_barrier(0x180);
      });
      uint32_t gm = __builtin_amdgcn_inverse_ballot_w64(a0) ? sw_gmax<8>(sc) : 0u;
      uint64_t bad = 0;
      if (last_live != a0) {
        bad = ends<false>(L, g.K, a0, last_live, gm);
        L.alive_m = last_live;  // the lanes live at the group's last step
      }
      // (empty asm: the compiler does not learn that a group without an end has nothing to remask -- it would
      // thread that path past the test, and the paths' join then costs nine register moves in each)
      asm("" : "+s"(bad));
      if (__builtin_expect(bad != 0, 0)) gm = remask<false>(L, g.K, a0, sc);
      fold(L, gm, t0, sc, 8u, c_of(g), g.K);
      t0 += 8u;
      g.A -= 8;
      if (!A7) g.C -= 8;  // (A7 reads c in the long branch only: from A's slot)
      k8 -= 8;
      // (empty asm: the key address is the one the loop carries -- otherwise it is re-based so that
      // the look-ahead costs a subtraction and a move)
      asm("" : "+v"(k8));
    } while (t0 <= te && L.alive_m);
  }

  // sweep: the chain steps 1 .. budget of chunk cc, while a lane's chain lasts
  __device__ __forceinline__ void sweep(Lane& L) {
    // Steps 1..8 as ONE masked group where the chain >> 2 snapshot is not before
    // step 8 (levels 5 and up): one address, one fold.  Level 4 (snapshot at
    // step 4) takes the pieces: the head, steps 2..4, and the blocks' groups
    // from step 5.
    const uint32_t base0 = Ring::base(cc, 0u, lane);
    const bool open8 = U8 || (budget_s >= 8u && budget >= 8u);  // wave-uniform
    if (open8) {
      if constexpr (U8) this->open8(L, at<8>(base0, 1u));
      else group_masked<8, true>(L, at<8>(base0, 1u), 1u);
      if (budget_s == 8u) L.snap();
    } else if constexpr (!U8) {
      group_masked<1, true>(L, at<1>(base0, 1u), 1u);
      if (budget_s == 1u) L.snap();
      if (budget >= 4u) {
        group_masked<3, false>(L, at<3>(base0, 2u), 2u);
        if (budget_s == 4u) L.snap();
      }
    }
    for (uint32_t b = 0; budget > 4u && L.alive_m; b++) {
      // block b = steps (64b, 64b + 64]: members k0 - 64b - 64 ... k0 - 64b + 62, i.e. the blocks b and b + 1 back
      const int blk = cc - (int)b - 1;
      if (b >= 1 && missing(blk)) {
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        build_blk(blk, fetch(64 * blk + (int)lane));
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
      }
      uint32_t ta = b == 0 ? (open8 ? 9u : 5u) : 64u * b + 1u;
      const uint32_t tb = min(64u * b + 64u, budget);
      const uint32_t base = Ring::base(cc, b, lane);
      if constexpr (U8) {
        // the snapshot is a group's end: the block's groups are walked up to it, and on from it
        while (ta <= tb && L.alive_m) {
          const bool cut = !L.snapped && budget_s <= tb;  // (budget_s >= ta: the steps before ta are done)
          const uint32_t te = cut ? budget_s : tb;
          run8(L, base, ta, te);
          if (cut) L.snap();
          ta = te + 1u;
        }
      } else {
        run(L, base, ta, tb);
      }
      if (tb >= budget) break;
    }
    if (!L.snapped) L.snap();  // every chain ended before step chain >> 2
  }

  // settle: the lane's result from its bests -- lengths from the scores,
  // distances from the members' positions
  __device__ __forceinline__ void settle(const Lane& L, uint2* out) const {
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    if (!L.own) return;
    const uint32_t p = L.p;
    uint32_t rx = 0, ry = 0;
    if (L.head) {
      uint32_t len = 2, dist = 0, len_s = 2, dist_s = 0;
      if (L.tail()) {  // maxc <= 12: min(lcp, maxc) exactly, first maximum in chain order (deflate.ts:1082-1105)
        const int k = this->k();
        uint32_t b = 2u << 16, bs = 2u << 16;
        for (uint32_t t = 1; t <= budget && (int)t <= k; t++) {
          const uint32_t q = member(t);
          const uint32_t key = (sw_hash(sw_word(win, q)) << 16) | q;
          if (t == 1u ? key < L.khead : key <= L.klim) break;
          // (three straight word compares.  sw_extend(win, p, q, maxc, 0) gives the same min(lcp, maxc), but its
          // loop inside this serial walk of up to chain steps cost 0.2 ms of level 6's sweep: DESIGN 4.2)
          uint32_t len = 12;
          for (uint32_t o = 0; o < 12u; o += 4) {
            const uint32_t y = sw_word(win, q + o) ^ sw_word(win, p + o);
            if (y) { len = o + (uint32_t)(__builtin_ctz(y) >> 3); break; }
          }
          const uint32_t sc = ((len < L.maxc ? len : L.maxc) << 16) | (0xffffu - t);
          b = max(b, sc);
          if (t <= budget_s) bs = max(bs, sc);
        }
        len = b >> 16;
        dist = len > 2u ? p - (uint32_t)mem[k - (int)(0xffffu - (b & 0xffffu))] : 0u;
        len_s = bs >> 16;
        dist_s = len_s > 2u ? p - (uint32_t)mem[k - (int)(0xffffu - (bs & 0xffffu))] : 0u;
      } else {
        const uint32_t tb = L.bt + 7u - (L.thr & 7u), tb_s = L.bt_s + 7u - (L.thr_s & 7u);  // the steps
        if (L.bt) {
          len = Sig::len(L.thr >> 3);
          dist = p - member(tb);
        }
        if (L.bt_s) {
          len_s = Sig::len(L.thr_s >> 3);
          dist_s = tb_s == tb ? dist : p - member(tb_s);
        }
        // long candidates beat every short one; a nice one's length was capped: measure it
        auto long_of = [&](uint32_t lt, uint32_t t, uint32_t& ln, uint32_t& ds) {
          const uint32_t q = member(t);
          ln = lt >> 3;
          if (ln >= L.nice) ln = sw_extend(win, p, q, L.maxc, Sig::EXT);
          ds = p - q;
        };
        if (L.lbt) long_of(L.lthr, L.lbt, len, dist);
        if (L.lbt_s) {
          if (L.lbt_s == L.lbt) {
            len_s = len;
            dist_s = dist;
          } else {
            long_of(L.lthr_s, L.lbt_s, len_s, dist_s);
          }
        }
      }
      rx = (len << 16) | (len > 2u ? dist : 0u) | (L.head & 0x8000u);
      ry = (len_s << 16) | (len_s > 2u ? dist_s : 0u);
    }
    out[p] = make_uint2(rx, ry);
  }
};

// The sweep of one window by one wave: results for the own positions
// [olo, ohi) of its members.  Chunks are claimed one ahead: the next chunk's
// members (its own and the block before) are loaded while this one is swept.
// PR: a wave claims runs [c, ce) of consecutive chunks, the next run during
// the last chunk of this one; only a run's first chunk needs the members of
// the block before.
template <bool A7, bool MW, bool PR, bool U8>
static __device__ __forceinline__ void sw_body(const uint32_t* win, void* ringp, uint16_t* mw, uint32_t* next,
                                               uint32_t n, uint32_t m, uint32_t olo, uint32_t ohi,
                                               const uint16_t* mem, uint2* out, int chain, int nice_cfg) {
  using Wave = SwWave<A7, MW, PR, U8>;
  const uint32_t lane = threadIdx.x & 63u;
  Wave W{win, (typename Wave::Ring*)ringp, mw, mem, n, m, lane, (uint32_t)chain, (uint32_t)chain >> 2,
         (uint32_t)nice_cfg, 0, zs_swr_empty(), 0};
  const uint32_t nchunks = (m + 63) / 64;
  auto claim = [&]() -> uint32_t {
    uint32_t c = 0;
    if (lane == 0) c = atomicAdd(next, 1u);
    return __builtin_amdgcn_readfirstlane(c);
  };
  auto claim_run = [&](uint32_t& c0, uint32_t& c1) {
    uint32_t a = 0, r = 0;
    if (lane == 0) {
      // (stale at worst: any length >= 1 is a valid run)
      const uint32_t cur = __hip_atomic_load(next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      r = zs_swr_run_len(cur < nchunks ? nchunks - cur : 0u, ZS_SW_RUN_CAP);
      a = atomicAdd(next, r);
    }
    c0 = __builtin_amdgcn_readfirstlane(a);
    c1 = min(c0 + (uint32_t)__builtin_amdgcn_readfirstlane(r), nchunks);
  };
  uint32_t c, ce = 0;
  if constexpr (PR) claim_run(c, ce);
  else c = claim();
  uint32_t pf_p = W.fetch((int)(64 * c + lane)), pf_b = W.fetch((int)(64 * c + lane) - 64);
  bool fresh_n = true;  // PR: the next chunk starts a run
  for (;;) {
    if (c >= nchunks) break;
    const bool fresh = fresh_n;  // (wave-uniform) a run's first chunk: pf_b was loaded, the ring holds nothing
    uint32_t cn, cen = ce;
    if constexpr (PR) {
      cn = c + 1u;
      fresh_n = cn >= ce;
      if (fresh_n) claim_run(cn, cen);
      if (fresh) W.vr = zs_swr_empty();
    } else {
      cn = claim();
    }
    W.cc = (int)c;
    const bool mem_ok = (uint32_t)W.k() < m;
    SW_STAT(0, 1);
    const uint32_t p = pf_p, qb = pf_b;  // (0 past the members)
    if (cn < nchunks) {
      pf_p = W.fetch((int)(64 * cn + lane));
      if (!PR || fresh_n) pf_b = W.fetch((int)(64 * cn + lane) - 64);
    }
    c = cn;
    ce = cen;
    // the lane's position is one of the window's own (a later window of a long
    // stream: its first 32,768 positions are look-back, candidates only)
    const bool own = mem_ok && p >= olo && p < ohi;
    // (PR: a chunk without own lanes builds nothing and breaks the ring's range -- the
    // next chunk with own lanes builds the block before it again.  In a window of zeros
    // that is 512 chunks of look-back skipped for one block rebuilt.)
    if (__builtin_amdgcn_ballot_w64(own) == 0) {
      W.vr = zs_swr_empty();
      continue;
    }
    typename Wave::Lane L;
    const uint4 rown = W.start(L, p, mem_ok, own);
    W.build(rown, p, qb, fresh);
    W.sweep(L);
    W.settle(L, out);
  }
}

template <bool U8>  // the host picks the instance from the level's chain (zs_sweep_uniform8)
__global__ __launch_bounds__(1024) void zs_k_sweep(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                   const uint32_t* __restrict__ in_len,
                                                   const uint64_t* __restrict__ pos_base,
                                                   const zs_sweep_seg* __restrict__ segs,
                                                   const uint16_t* __restrict__ members, uint2* __restrict__ mres,
                                                   int chain, int nice_cfg) {
  // the rings (and level 7's member windows), laid over each other: one form runs per launch
  constexpr uint32_t RING_BYTES = 16u * sizeof(SwRing), MWIN_BYTES = 16u * ZS_SW_MW * sizeof(uint16_t);
  static_assert(16u * sizeof(SwRingP) <= RING_BYTES + MWIN_BYTES, "the persistent rings must fit the old ones' LDS");
  __shared__ __attribute__((aligned(16))) uint8_t rmem[RING_BYTES + MWIN_BYTES];
  __shared__ __attribute__((aligned(16))) uint32_t win[ZS_SW_WIN_WORDS];
  __shared__ uint32_t next;
  const zs_sweep_seg G = segs[blockIdx.x];
  const int s = (int)G.s;
  const uint32_t n = in_len[s] - G.base;  // bytes from the window's start to the stream's end
  if (n < 3) return;
  const uint32_t m = min(n - 2, G.ohi);
  const uint8_t* src = in + in_off[s] + G.base;
  // the window in LDS, zero padded past the stream's end (reads run up to 16
  // bytes past a longest match); the OR of its bytes' top bits picks the
  // signature form
  uint32_t hi = 0;
  if ((((uintptr_t)src) & 15u) == 0) {
    for (uint32_t i = threadIdx.x; 4 * i < ZS_SW_WIN_WORDS; i += 1024) {
      const uint32_t b = 16 * i;
      uint4 v;
      if (b + 16 <= n) v = ((const uint4*)src)[i];
      else {
        uint32_t t[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < 16; k++)
          if (b + k < n) t[k >> 2] |= (uint32_t)src[b + k] << (8 * (k & 3));
        v = make_uint4(t[0], t[1], t[2], t[3]);
      }
      hi |= v.x | v.y | v.z | v.w;
      if (4 * i + 3 < ZS_SW_WIN_WORDS) *(uint4*)(win + 4 * i) = v;
      else for (uint32_t k = 0; 4 * i + k < ZS_SW_WIN_WORDS; k++) win[4 * i + k] = (&v.x)[k];
    }
  } else {
    for (uint32_t i = threadIdx.x; i < ZS_SW_WIN_WORDS; i += 1024) {
      uint32_t v = 0;
      for (uint32_t k = 0; k < 4; k++)
        if (4 * i + k < n) v |= (uint32_t)src[4 * i + k] << (8 * k);
      hi |= v;
      win[i] = v;
    }
  }
  if (threadIdx.x == 0) next = 0;
  const bool a7 = !__syncthreads_or((hi & 0x80808080u) != 0);
  const uint32_t wave = threadIdx.x >> 6;
  const uint16_t* mem = members + G.mb;
  uint2* out = mres + pos_base[s] + G.base;
  const uint32_t olo = G.olo, ohi = G.ohi;
  if (chain <= (int)ZS_SWR_MAX_CHAIN) {  // levels 4..6: the persistent ring
    SwRingP* const R = reinterpret_cast<SwRingP*>(rmem) + wave;
    if (a7) sw_body<true, false, true, U8>(win, R, nullptr, &next, n, m, olo, ohi, mem, out, chain, nice_cfg);
    else sw_body<false, false, true, U8>(win, R, nullptr, &next, n, m, olo, ohi, mem, out, chain, nice_cfg);
    return;
  }
  SwRing* const R = reinterpret_cast<SwRing*>(rmem) + wave;
  uint16_t* const mw = reinterpret_cast<uint16_t*>(rmem + RING_BYTES) + wave * ZS_SW_MW;
  if (chain + 64 <= (int)ZS_SW_MW) {  // level 7
    if (a7) sw_body<true, true, false, U8>(win, R, mw, &next, n, m, olo, ohi, mem, out, chain, nice_cfg);
    else sw_body<false, true, false, U8>(win, R, mw, &next, n, m, olo, ohi, mem, out, chain, nice_cfg);
  } else {  // levels 8, 9: positions from HBM
    if (a7) sw_body<true, false, false, U8>(win, R, mw, &next, n, m, olo, ohi, mem, out, chain, nice_cfg);
    else sw_body<false, false, false, U8>(win, R, mw, &next, n, m, olo, ohi, mem, out, chain, nice_cfg);
  }
}
template __global__ void zs_k_sweep<true>(const uint8_t*, const uint64_t*, const uint32_t*, const uint64_t*,
                                          const zs_sweep_seg*, const uint16_t*, uint2*, int, int);
template __global__ void zs_k_sweep<false>(const uint8_t*, const uint64_t*, const uint32_t*, const uint64_t*,
                                           const zs_sweep_seg*, const uint16_t*, uint2*, int, int);
