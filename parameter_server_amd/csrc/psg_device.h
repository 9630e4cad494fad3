// psg_device.h -- device helpers shared by the gfx950 kernels: the one
// definition of each leaf primitive.  Kernel files pull
// the names in inside their anonymous namespace and do not redefine them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AS1 __attribute__((address_space(1)))

namespace psg {
namespace dev {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// global (not flat) accesses: a flat access also counts on lgkmcnt, so a
// kernel's LDS waits would wait for its loads in flight too
template <typename T>
__device__ __forceinline__ const AS1 T* G(const T* p) {
  return (const AS1 T*)p;
}
template <typename T>
__device__ __forceinline__ AS1 T* GW(T* p) {
  return (AS1 T*)p;
}

// a wave-uniform value into scalar registers
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}

// the lane index recomputed from nothing (mbcnt over a full mask), so a value
// needed late in the kernel does not keep the thread-id register live (at 64
// VGPRs it is the value that would be spilled to scratch: HBM writes)
__device__ __forceinline__ uint32_t lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// std::min(a, b) / std::max(a, b) as <algorithm> defines them: b < a ? b : a
// and a < b ? b : a.  Not fmin / fmax: a NaN first argument stays a NaN, as
// in the reference.
__device__ __forceinline__ double std_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double std_max(double a, double b) { return a < b ? b : a; }

// blocks b and b+8 share an XCD (observed dispatch, speed only): block b of n
// takes index xcd_index(b, n), which gives each XCD a contiguous run of
// indices (tiles, chunks), so the cache lines two neighbours share are read
// once.  A permutation of [0, n).
__host__ __device__ constexpr __forceinline__ uint32_t xcd_index(uint32_t b, uint32_t n) {
  const uint32_t x = b & 7u, j = b >> 3, q = n >> 3, r = n & 7u;
  return x * q + (x < r ? x : r) + j;
}
constexpr bool xcd_index_permutes(uint32_t n) {  // n <= 64
  uint64_t seen = 0;
  for (uint32_t b = 0; b < n; ++b) {
    const uint32_t i = xcd_index(b, n);
    if (i >= n || (seen >> i & 1u)) return false;
    seen |= 1ull << i;
  }
  return true;
}
// every remainder edge r = n & 7
static_assert(xcd_index_permutes(1) && xcd_index_permutes(7) && xcd_index_permutes(8) &&
                  xcd_index_permutes(9) && xcd_index_permutes(15) && xcd_index_permutes(16) &&
                  xcd_index_permutes(17) && xcd_index_permutes(64),
              "xcd_index: a permutation of [0, n)");

// inclusive 64-lane prefix sum by DPP (row shifts, then row broadcasts):
// immediate lane controls, so no per-lane shuffle addresses stay live (the
// __shfl_up form kept six address VGPRs alive across the kernel and spilled
// them at 8 waves/SIMD)
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return x;
}

// 16 B per lane from global memory straight into LDS (gfx950 LDS-DMA): lane l
// writes lds + 16 l; nontemporal (the tile kernels' D is read by one tile)
// Issued by inline asm (M0 saved and restored, as the compiler reserves it):
// the builtin form made the compiler's wait-count pass wait for the DMA at
// the next reuse of its address registers, i.e. right after issuing it.  The
// compiler does not see these loads, so readers of the LDS they fill wait
// for them explicitly (dma_wait); its own vmcnt waits stay correct, only
// more conservative (the DMAs are older than its loads).
typedef __attribute__((address_space(3))) void* LdsPtr;
__device__ __forceinline__ void dma16(const void* g, void* lds) {
  const uint32_t la = (uint32_t)(uintptr_t)(LdsPtr)lds;
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(g), "s"(la)
      : "memory");
}
__device__ __forceinline__ void dma_wait() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// a workgroup barrier that makes LDS writes visible but leaves vector-memory
// operations (LDS-DMA, loads) in flight: __syncthreads() would wait for them
// (its release fence waits vmcnt(0) while an LDS-DMA is pending)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0); vmcnt and expcnt not waited for
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The tile kernels' search window: consecutive 8-B keys of the LDS image of D
// from one slot on.  Written as plain loads, the compiler fuses each pair
// into one two-address ds_read2_b64, which the LDS serves as two accesses of
// 4 lane groups at 32-bank mapping: 8 LDS-array cycles per pair, where a
// ds_read_b64 takes 2 and a ds_read_b128 4 (64-bank mapping), i.e. 16 cycles
// for a 32-B window that needs 8.  The forms (PSG_LDSWIN, A/B builds;
// profiles/ldswin_ab.txt):
//   0  plain loads (fused)
//   1  single-address ds_read_b64 in one asm statement.  The compiler does
//      not count LDS reads issued by asm, so the statement waits for them
//      itself, its outputs are early-clobber and it orders itself against
//      the compiler's LDS accesses ("memory")
//   2  (4 keys) the window start rounded down to even, read as two 16-B
//      aligned ds_read_b128: lds_window4 returns that start, and the caller
//      counts from it (the key before an odd bucket start lies in an earlier
//      bucket, so it is below every key of this one)
//   3  single-address ds_read_b64 the compiler issues and counts itself:
//      each from its own copy of the address, made opaque by an empty asm
//      statement, so no two share a base register to be fused on
#ifndef PSG_LDSWIN
#define PSG_LDSWIN 1
#endif
constexpr bool kWindowEven = PSG_LDSWIN == 2;
typedef __attribute__((address_space(3))) const uint64_t* LdsKeys;
__device__ __forceinline__ void lds_window2(const uint64_t* dk, uint32_t l, uint64_t& k0,
                                            uint64_t& k1) {
#if PSG_LDSWIN == 1
  const uint32_t a = (uint32_t)(uintptr_t)(LdsPtr)(dk + l);
  asm volatile(
      "ds_read_b64 %0, %2\n\tds_read_b64 %1, %2 offset:8\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(k0), "=&v"(k1)
      : "v"(a)
      : "memory");
#elif PSG_LDSWIN == 3
  LdsKeys q = (LdsKeys)(dk + l);
  k0 = q[0];
  asm("" : "+v"(q));
  k1 = q[1];
#else
  k0 = dk[l];
  k1 = dk[l + 1];
#endif
}
__device__ __forceinline__ uint32_t lds_window4(const uint64_t* dk, uint32_t l, uint64_t& k0,
                                                uint64_t& k1, uint64_t& k2, uint64_t& k3) {
#if PSG_LDSWIN == 1
  const uint32_t a = (uint32_t)(uintptr_t)(LdsPtr)(dk + l);
  asm volatile(
      "ds_read_b64 %0, %4\n\tds_read_b64 %1, %4 offset:8\n\t"
      "ds_read_b64 %2, %4 offset:16\n\tds_read_b64 %3, %4 offset:24\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(k0), "=&v"(k1), "=&v"(k2), "=&v"(k3)
      : "v"(a)
      : "memory");
#elif PSG_LDSWIN == 2
  l &= ~1u;
  const u64x2 x0 = *(const u64x2*)&dk[l], x1 = *(const u64x2*)&dk[l + 2];
  k0 = x0.x; k1 = x0.y; k2 = x1.x; k3 = x1.y;
#elif PSG_LDSWIN == 3
  LdsKeys q = (LdsKeys)(dk + l);
  k0 = q[0];
  asm("" : "+v"(q));
  k1 = q[1];
  asm("" : "+v"(q));
  k2 = q[2];
  asm("" : "+v"(q));
  k3 = q[3];
#else
  k0 = dk[l]; k1 = dk[l + 1]; k2 = dk[l + 2]; k3 = dk[l + 3];
#endif
  return l;
}

// ----------------------------------------------------------------------
// wave-cooperative k-ary search: first index i in [0, n) whose key
// satisfies (upper ? S[i] > key : S[i] >= key); n if none.  64 probes per
// round -> ceil(log64 n)+1 dependent global loads instead of log2 n.
// Every lane of the wave must call it with the same arguments.
// ----------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_search(const uint64_t* __restrict__ S,
                                                uint64_t n, uint64_t key,
                                                bool upper, int lane) {
  uint64_t lo = 0, hi = n;  // answer in [lo, hi]
  while (hi > lo) {
    const uint64_t len = hi - lo;
    const uint64_t step = (len + 63) >> 6;
    const uint64_t idx = lo + (uint64_t)(lane + 1) * step - 1;
    bool pred = true;  // probes past the range count as "true"
    if (idx < hi) {
      const uint64_t s = S[idx];
      pred = upper ? (s > key) : (s >= key);
    }
    const unsigned long long mask = __ballot(pred);
    if (mask == 0) {
      lo = hi;
      break;
    }
    const uint64_t f = (uint64_t)(__ffsll((long long)mask) - 1);
    const uint64_t nlo = lo + f * step;
    uint64_t nhi = lo + (f + 1) * step - 1;
    if (nhi > hi) nhi = hi;
    lo = nlo;
    hi = nhi;
  }
  return lo;
}

// lower_bound(S, xl) inside a bracket with S[a] < xl <= S[c]: interpolation
// probes (pushes of murmur-hashed keys are near-uniform), bisection, then
// the last <= 15 candidates in one round trip.  One lane per search.
__device__ __forceinline__ uint64_t bracket_lower_bound(const uint64_t* S, uint64_t xl,
                                                        uint64_t a, uint64_t c, uint64_t ka,
                                                        uint64_t kc) {
  for (int it = 0; it < 6 && c - a > 16u; ++it) {
    const double f = (double)(xl - ka) / (double)(kc - ka);
    uint64_t mid = a + 1 + (uint64_t)(f * (double)(c - a - 1));
    mid = mid < c ? mid : c - 1;
    const uint64_t km = S[mid];
    if (km < xl) {
      a = mid;
      ka = km;
    } else {
      c = mid;
      kc = km;
    }
  }
  while (c - a > 16u) {
    const uint64_t mid = a + ((c - a) >> 1);
    if (S[mid] < xl) a = mid; else c = mid;
  }
  // independent loads of S[a+1 .. c-1] (indices clamped to c, where
  // S[c] >= xl counts 0)
  uint32_t below = 0;
#pragma unroll
  for (uint32_t i = 1; i < 16u; ++i) {
    const uint64_t idx = a + i < c ? a + i : c;
    below += S[idx] < xl ? 1u : 0u;
  }
  return a + 1u + below;
}

// lower_bound(S[0, n), x) by bracket_lower_bound: in [0, n] whatever S holds
__device__ __forceinline__ uint64_t interp_lower_bound(const uint64_t* S, uint64_t n, uint64_t x) {
  if (n == 0) return 0;
  const uint64_t k0 = S[0], kn = S[n - 1];
  if (x <= k0) return 0;
  if (x > kn) return n;
  return bracket_lower_bound(S, x, 0, n - 1, k0, kn);
}

// lower_bound over a sorted LDS array of n <= 2*TILE-1 keys: fixed trip
// count (log2(TILE)+1 probes), so the wave never diverges on the loop.
template <int TILE>
__device__ __forceinline__ int lds_lower_bound(const uint64_t* a, int n,
                                               uint64_t k) {
  int pos = 0;
#pragma unroll
  for (int step = TILE; step > 0; step >>= 1) {
    const int c = pos + step;
    if (c <= n && a[c - 1] < k) pos = c;
  }
  return pos;
}

__device__ __forceinline__ uint64_t gl_lower_bound(const uint64_t* __restrict__ a,
                                                   uint64_t n, uint64_t k) {
  uint64_t lo = 0, len = n;
  while (len > 0) {
    const uint64_t half = len >> 1;
    if (a[lo + half] < k) {
      lo += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return lo;
}

// Exclusive scan across an NT-thread workgroup.  wsum: LDS scratch of NT/64
// words.  Contains two barriers; callers separate consecutive uses with a
// barrier of their own.
template <int NT>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum,
                                                    uint32_t* total) {
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  constexpr int kW = NT / 64;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  if (w == 0) {
    uint32_t s = lane < kW ? wsum[lane] : 0u;
#pragma unroll
    for (int d = 1; d < kW; d <<= 1) {
      const uint32_t y = __shfl_up(s, d, 64);
      if (lane >= d) s += y;
    }
    if (lane < kW) wsum[lane] = s;
  }
  __syncthreads();
  *total = wsum[kW - 1];
  return (w > 0 ? wsum[w - 1] : 0u) + x - v;
}

// The fixed-order sum every device objv is built on (psg_mb_gradient,
// psg_mb_darling_objv, psg_darling_progress): the tree sum of a 256-thread
// workgroup's values v, over s (256 doubles of LDS); s[0] on return, for
// thread 0 to read.  The result's bits depend on this order: change it for
// all callers or for none.
__device__ __forceinline__ void block_tree_sum(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
    __syncthreads();
  }
}

// Scale of the tile kernels' bucket map bucket(x) = umulhi(x, mul): every
// x <= r32 (< 2^32) lands below nb.  An f32 reciprocal with a 2^-20 margin
// (reciprocal ~2^-23, conversions and products 2^-24 each) replaces the
// 64-bit integer division floor(nb * 2^32 / (r32 + 1)), which compiles to a
// ~100-instruction scalar routine in every wave; only the spread of keys over
// buckets depends on the exact value, not what a search finds.
__device__ __forceinline__ uint32_t bucket_scale(uint64_t r32, uint32_t nb) {
  const float f = (float)nb * 4294967296.0f * (1.0f - 0x1p-20f) *
                  __builtin_amdgcn_rcpf((float)(r32 + 1ull));
  return f >= 4294967295.0f ? 0xffffffffu : (uint32_t)f;
}

// ----------------------------------------------------------------------
// A plan's resident bucket index (psg_tile.hip bucket_index_kernel): per
// tile of kNB buckets, kNB / 2 bytes; nibble b (bits 4 (b % 8) of u32 word
// b / 8) is the number of server keys in bucket b, 0..14.  A first nibble of
// 15 marks a tile whose table is not stored (a bucket of more than 14 keys):
// its kernels build the table themselves, as without an index.
// One wave decodes a tile: lane l holds the kNB / 64 nibbles of buckets
// [l kNB / 64, (l + 1) kNB / 64), loaded by bucket_index_load; the bucket
// starts are the running sum of the counts (an in-lane prefix on packed
// bytes, then one wave scan).
// ----------------------------------------------------------------------
template <int kNB>
struct BucketIndexWords {
  static_assert(kNB == 1024 || kNB == 2048 || kNB == 4096, "8, 16 or 32 B per lane");
  uint32_t x[kNB / 512];
};

template <int kNB>
__device__ __forceinline__ BucketIndexWords<kNB> bucket_index_load(const uint32_t* ix, int lane) {
  BucketIndexWords<kNB> r;
  if constexpr (kNB == 1024) {
    const u32x2 a = __builtin_nontemporal_load((const AS1 u32x2*)ix + lane);
    r.x[0] = a.x; r.x[1] = a.y;
  } else {
#pragma unroll
    for (int i = 0; i < kNB / 2048; ++i) {
      const u32x4 a =
          __builtin_nontemporal_load((const AS1 u32x4*)ix + lane * (kNB / 2048) + i);
      r.x[4 * i] = a.x; r.x[4 * i + 1] = a.y; r.x[4 * i + 2] = a.z; r.x[4 * i + 3] = a.w;
    }
  }
  return r;
}

// Called by every lane of ONE wave with the words of bucket_index_load:
// writes the kNB u16 bucket starts to bt32 (as the kernels' tables: u16 b at
// half b of the array), and the word past them: bt[kNB] = nt (the end of the
// last bucket), bt[kNB + 1] = 1 iff the tile is marked -- then the table is
// zeroed instead, a cleared histogram for the caller's own build.  The
// caller's next workgroup barrier publishes all of it; bucket_index_marked
// reads the flag back (workgroup-uniform).
template <int kNB>
__device__ __forceinline__ void bucket_index_decode(const BucketIndexWords<kNB>& ix,
                                                    uint32_t* bt32, uint32_t nt, int lane) {
  constexpr int W = kNB / 512;
  const bool marked = ((uint32_t)__builtin_amdgcn_readfirstlane((int)ix.x[0]) & 15u) == 15u;
  // per word, on packed bytes (8 counts <= 14: sums below 256): ev/od byte j
  // = the counts of the word before nibble 2j / 2j + 1
  uint32_t ev[W], od[W], before[W], tot = 0;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const uint32_t lo = ix.x[i] & 0x0f0f0f0fu, hi = (ix.x[i] >> 4) & 0x0f0f0f0fu;
    const uint32_t s = (lo + hi) * 0x01010101u;  // byte j: counts through nibble 2j + 1
    ev[i] = s - lo - hi;
    od[i] = s - hi;
    before[i] = tot;
    tot += s >> 24;
  }
  const uint32_t off = wave_scan_incl(tot) - tot;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const uint32_t base = (off + before[i]) * 0x00010001u;  // starts <= nt < 2^16: no carry
    u32x4 o;
    o.x = ((ev[i] & 0xffu) | (od[i] & 0xffu) << 16) + base;
    o.y = ((ev[i] >> 8 & 0xffu) | (od[i] >> 8 & 0xffu) << 16) + base;
    o.z = ((ev[i] >> 16 & 0xffu) | (od[i] >> 16 & 0xffu) << 16) + base;
    o.w = ((ev[i] >> 24) | (od[i] >> 24) << 16) + base;
    if (marked) o = u32x4{0u, 0u, 0u, 0u};
    *(u32x4*)&bt32[4 * (lane * W + i)] = o;
  }
  if (lane == 0) bt32[kNB / 2] = nt | (marked ? 0x10000u : 0u);
}

template <int kNB>
__device__ __forceinline__ bool bucket_index_marked(const uint32_t* bt32) {
  return ((uint32_t)__builtin_amdgcn_readfirstlane((int)bt32[kNB / 2]) >> 16) != 0u;
}

// One step of the per-key fold in push-arrival order.  p = push index in
// this launch, lp = last push index in this launch that held the key (-1:
// none yet).  Serial (the reference default) adds +0.0 for every absent
// later push (kv_vector.h:200); since x + 0.0 == x except -0.0 -> +0.0 and
// the operation is idempotent, one "+ 0" per run of absent pushes is exact.
template <typename V>
__device__ __forceinline__ V fold_step(V acc, int lp, int p, V v,
                                       bool parallel, bool cont) {
  if (p == 0 && !cont) return v;  // the first push is assigned (:195-196)
  if (!parallel) {
    const bool gap = (lp >= 0) ? (p - lp > 1) : (cont && p > 0);
    if (gap) acc = acc + V(0);
  }
  return acc + v;
}

}  // namespace dev
}  // namespace psg
