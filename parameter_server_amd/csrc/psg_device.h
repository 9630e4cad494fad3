// psg_device.h -- device helpers shared by the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psg {
namespace dev {

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
  typedef uint32_t v2 __attribute__((ext_vector_type(2)));
  typedef uint32_t v4 __attribute__((ext_vector_type(4)));
  BucketIndexWords<kNB> r;
  if constexpr (kNB == 1024) {
    const v2 a = __builtin_nontemporal_load(
        (const __attribute__((address_space(1))) v2*)ix + lane);
    r.x[0] = a.x; r.x[1] = a.y;
  } else {
#pragma unroll
    for (int i = 0; i < kNB / 2048; ++i) {
      const v4 a = __builtin_nontemporal_load(
          (const __attribute__((address_space(1))) v4*)ix + lane * (kNB / 2048) + i);
      r.x[4 * i] = a.x; r.x[4 * i + 1] = a.y; r.x[4 * i + 2] = a.z; r.x[4 * i + 3] = a.w;
    }
  }
  return r;
}

// inclusive 64-lane prefix sum by DPP (row shifts, then row broadcasts)
__device__ __forceinline__ uint32_t wave_scan_incl_dpp(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return x;
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
  typedef uint32_t v4 __attribute__((ext_vector_type(4)));
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
  const uint32_t off = wave_scan_incl_dpp(tot) - tot;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const uint32_t base = (off + before[i]) * 0x00010001u;  // starts <= nt < 2^16: no carry
    v4 o;
    o.x = ((ev[i] & 0xffu) | (od[i] & 0xffu) << 16) + base;
    o.y = ((ev[i] >> 8 & 0xffu) | (od[i] >> 8 & 0xffu) << 16) + base;
    o.z = ((ev[i] >> 16 & 0xffu) | (od[i] >> 16 & 0xffu) << 16) + base;
    o.w = ((ev[i] >> 24) | (od[i] >> 24) << 16) + base;
    if (marked) o = v4{0u, 0u, 0u, 0u};
    *(v4*)&bt32[4 * (lane * W + i)] = o;
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
