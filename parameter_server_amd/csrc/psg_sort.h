// psg_sort.h -- the device sort and scan layer of psg_worker.hip and
// psg_auc.hip: the stable 8-bit LSD radix passes over 64-bit keys with a
// 32-bit payload (DESIGN.md 4.8 a), the count / scan / emit of a flag over a
// sorted array (4.8 b), the binary search and the wave's fold of a run's
// labels.  It stands alone (but for psg_device.h's block map): the sort's
// shape is defined here, once, and psg_mb_sort_tile() reports it;
// tests/worker_ref.py mirrors it.  Kernels are file-local in each
// translation unit that includes this (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psg.h"
#include "psg_device.h"
#include "psg_host.h"

#ifndef PSG_SORT_KPT
#define PSG_SORT_KPT 8  // A/B builds: 4, 16, 32
#endif

namespace psg {
namespace {

constexpr int kSortKPT = PSG_SORT_KPT;           // pairs per lane per tile
constexpr uint32_t kSortTile = 256 * kSortKPT;   // pairs per workgroup
constexpr uint32_t kWaveSpan = 64 * kSortKPT;    // pairs per wave
constexpr uint32_t kFlagTile = 2048;             // elements per workgroup of the flag scans

// XCD-contiguous runs of consecutive tiles: tiles next to each other write
// next to each other in every digit's output range, and their partial lines
// meet in one XCD's L2
using dev::xcd_index;

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
  for (uint32_t s = 1; s < 64; s <<= 1) {
    const uint32_t u = __shfl_up(v, s, 64);
    if (lane >= s) v += u;
  }
  return v;
}

// exclusive scan of v over the 256 lanes of the workgroup; ws: 4 LDS words
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t* ws, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_scan(v, lane);
  __syncthreads();
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  uint32_t b = 0, t = 0;
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t x = ws[i];
    if (i < w) b += x;
    t += x;
  }
  *total = t;
  return b + inc - v;
}

// workgroup r: c[r * n .. + n) becomes its exclusive scan, total[r] its sum
__global__ __launch_bounds__(256) void row_scan_kernel(uint32_t* __restrict__ c, uint32_t n,
                                                       uint32_t* __restrict__ total) {
  __shared__ uint32_t ws[4];
  uint32_t* row = c + (size_t)blockIdx.x * n;
  uint32_t carry = 0;
  for (uint32_t b = 0; b < n; b += 256) {
    const uint32_t i = b + threadIdx.x;
    const uint32_t v = i < n ? row[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exscan(v, ws, &tot);
    if (i < n) row[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

// first index of k[0 .. n) that holds `key` or more
template <class T>
__device__ __forceinline__ uint32_t lower_bound(const T* __restrict__ k, uint32_t n, T key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (k[mid] < key) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// One lane per sorted item, r its run.  The lanes of a wave that share a run
// (they are neighbours) fold their labels with ballots: true in the first
// lane of each such group, with the group's positives and negatives.  Every
// lane of the wave comes here.
__device__ __forceinline__ bool run_label_counts(uint32_t r, bool valid, bool positive,
                                                 uint32_t lane, uint32_t* cp, uint32_t* cn) {
  const uint32_t rprev = __shfl_up(r, 1, 64);
  const bool head = valid && (lane == 0 || r != rprev);
  const uint64_t heads = __ballot(head), posb = __ballot(positive), val = __ballot(valid);
  if (head) {
    const uint64_t above = heads & ~((2ull << lane) - 1);  // the groups after this one
    const int end = above ? __ffsll((unsigned long long)above) - 1 : 64;
    const uint64_t upto = end == 64 ? ~0ull : (1ull << end) - 1;
    const uint64_t seg = upto & ~((1ull << lane) - 1) & val;
    *cp = (uint32_t)__popcll(seg & posb);
    *cn = (uint32_t)__popcll(seg) - *cp;
  }
  return head;
}

// the valid lanes of the wave whose digit equals this lane's
__device__ __forceinline__ uint64_t match_digit(uint32_t d, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// ---- (a) ------------------------------------------------------------------
// orand[0] |= every key, orand[1] &= every key
__global__ __launch_bounds__(256) void key_bits_kernel(const uint64_t* __restrict__ keys,
                                                       uint32_t n,
                                                       unsigned long long* __restrict__ orand) {
  uint64_t o = 0, a = ~0ull;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256u) {
    const uint64_t k = keys[i];
    o |= k;
    a &= k;
  }
  for (int s = 32; s >= 1; s >>= 1) {
    o |= __shfl_xor(o, s, 64);
    a &= __shfl_xor(a, s, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicOr(orand, (unsigned long long)o);
    atomicAnd(orand + 1, (unsigned long long)a);
  }
}

// counts[d * ntiles + t] = pairs of tile t whose digit is d
__global__ __launch_bounds__(256) void sort_count_kernel(const uint64_t* __restrict__ keys,
                                                         uint32_t n, int shift,
                                                         uint32_t* __restrict__ counts,
                                                         uint32_t ntiles) {
  __shared__ uint32_t h[256];
  const uint32_t t = xcd_index(blockIdx.x, gridDim.x);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)t * kSortTile + (uint64_t)w * kWaveSpan + lane;
#pragma unroll 4
  for (int j = 0; j < kSortKPT; ++j) {
    const uint64_t i = base + (uint64_t)j * 64u;
    const bool valid = i < n;
    const uint32_t d = valid ? (uint32_t)(keys[i] >> shift) & 255u : 0u;
    const uint64_t m = match_digit(d, valid);
    if (valid && (m & ((1ull << lane) - 1)) == 0)  // first lane of its group
      atomicAdd(&h[d], (uint32_t)__popcll(m));
  }
  __syncthreads();
  counts[(size_t)threadIdx.x * ntiles + t] = h[threadIdx.x];
}

// pin null: the positions are 0 .. n-1 (the first pass)
__global__ __launch_bounds__(256) void sort_scatter_kernel(
    const uint64_t* __restrict__ kin, const uint32_t* __restrict__ pin, uint64_t* __restrict__ kout,
    uint32_t* __restrict__ pout, uint32_t n, int shift, const uint32_t* __restrict__ counts,
    const uint32_t* __restrict__ dtotal, uint32_t ntiles) {
  __shared__ uint32_t cnt[4][256];
  __shared__ uint32_t dbase[256];
  __shared__ uint32_t ws[4];
  const uint32_t t = xcd_index(blockIdx.x, gridDim.x);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  for (int i = 0; i < 4; ++i) cnt[i][tid] = 0;
  {  // first output index of digit `tid` for this tile
    uint32_t tot;
    const uint32_t ex = block_exscan(dtotal[tid], ws, &tot);
    dbase[tid] = ex + counts[(size_t)tid * ntiles + t];
  }
  __syncthreads();
  // The wave's counters are read by every lane and then advanced by one lane
  // per group.  LDS operations of one wave run in order, so a step reads
  // what the step before wrote; volatile keeps the compiler from carrying a
  // counter in a register across steps.
  volatile uint32_t* mine = cnt[w];
  const uint64_t base = (uint64_t)t * kSortTile + (uint64_t)w * kWaveSpan + lane;
  uint64_t key[kSortKPT];
  uint32_t off[kSortKPT];
#pragma unroll
  for (int j = 0; j < kSortKPT; ++j) {
    const uint64_t i = base + (uint64_t)j * 64u;
    const bool valid = i < n;
    key[j] = valid ? kin[i] : 0;
    const uint32_t d = (uint32_t)(key[j] >> shift) & 255u;
    const uint64_t m = match_digit(d, valid);
    const uint32_t before = mine[d];  // the wave's earlier steps
    const uint32_t below = (uint32_t)__popcll(m & ((1ull << lane) - 1));
    const uint32_t group = (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
    if (valid && below + 1 == group) mine[d] = before + group;  // last lane of the group
    __builtin_amdgcn_wave_barrier();
    off[j] = before + below;
  }
  __syncthreads();
  {  // the waves' totals of digit `tid` become their exclusive prefix
    uint32_t run = 0;
    for (int i = 0; i < 4; ++i) {
      const uint32_t x = cnt[i][tid];
      cnt[i][tid] = run;
      run += x;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSortKPT; ++j) {
    const uint64_t i = base + (uint64_t)j * 64u;
    if (i < n) {
      const uint32_t d = (uint32_t)(key[j] >> shift) & 255u;
      const uint32_t dst = dbase[d] + cnt[w][d] + off[j];
      if (dst < n) {  // always, by the counts; keeps a bad count in bounds
        kout[dst] = key[j];
        pout[dst] = pin ? pin[i] : (uint32_t)i;
      }
    }
  }
}

// no digit differs: the input order is the sorted order
__global__ __launch_bounds__(256) void sort_identity_kernel(const uint64_t* __restrict__ kin,
                                                            uint64_t* __restrict__ kout,
                                                            uint32_t* __restrict__ pout,
                                                            uint32_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) {
    kout[i] = kin[i];
    pout[i] = (uint32_t)i;
  }
}

// ---- flag scans: (b) and the compaction of (c) -----------------------------
// A lane owns 8 consecutive elements of a 2048-element tile.
struct HeadFlag {  // element i starts a run of the sorted keys
  const uint64_t* k;
  __device__ bool operator()(uint32_t i) const { return i == 0 || k[i] != k[i - 1]; }
};

template <class Flag>
__global__ __launch_bounds__(256) void flag_count_kernel(Flag f, uint32_t n,
                                                         uint32_t* __restrict__ tile_sum) {
  __shared__ uint32_t ws[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kFlagTile + threadIdx.x * 8u;
  uint32_t c = 0;
  for (uint32_t j = 0; j < 8; ++j)
    if (i0 + j < n) c += f((uint32_t)(i0 + j)) ? 1u : 0u;
  uint32_t tot;
  (void)block_exscan(c, ws, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

struct HeadEmit {  // ex: run heads before element i
  const uint64_t* k;
  uint64_t* uniq_key;
  uint32_t* run_start;  // [n_uniq + 1]
  uint32_t* run_of;     // [n]
  __device__ void operator()(uint32_t i, uint32_t ex, bool head, uint32_t n) const {
    if (head) {
      uniq_key[ex] = k[i];
      run_start[ex] = i;
    }
    const uint32_t after = ex + (head ? 1u : 0u);
    run_of[i] = after - 1;  // i == 0 is a head: after >= 1
    if (i == n - 1) run_start[after] = n;
  }
};

template <class Flag, class Emit>
__global__ __launch_bounds__(256) void flag_emit_kernel(Flag f, Emit e, uint32_t n,
                                                        const uint32_t* __restrict__ tile_base) {
  __shared__ uint32_t ws[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kFlagTile + threadIdx.x * 8u;
  bool fl[8];
  uint32_t c = 0;
  for (uint32_t j = 0; j < 8; ++j) {
    fl[j] = i0 + j < n && f((uint32_t)(i0 + j));
    c += fl[j] ? 1u : 0u;
  }
  uint32_t tot;
  uint32_t ex = tile_base[blockIdx.x] + block_exscan(c, ws, &tot);
  for (uint32_t j = 0; j < 8; ++j)
    if (i0 + j < n) {
      e((uint32_t)(i0 + j), ex, fl[j], n);
      ex += fl[j] ? 1u : 0u;
    }
}

inline uint32_t blocks_of(uint64_t n, uint64_t per) { return (uint32_t)((n + per - 1) / per); }
#define LAUNCH(kernel, grid, s, ...) \
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, __VA_ARGS__)

inline int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PSG_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
  return PSG_OK;
}

// n elements: e(i, flagged elements before i, f(i), n) for every i, and
// *total = the flagged elements; tile_sum: blocks_of(n, kFlagTile) words
template <class Flag, class Emit>
void enqueue_flag_scan(Flag f, Emit e, uint32_t n, uint32_t* tile_sum, uint32_t* total,
                       hipStream_t s) {
  const uint32_t nt = blocks_of(n, kFlagTile);
  LAUNCH(flag_count_kernel<Flag>, nt, s, f, n, tile_sum);
  LAUNCH(row_scan_kernel, 1, s, tile_sum, nt, total);
  LAUNCH((flag_emit_kernel<Flag, Emit>), nt, s, f, e, n, tile_sum);
}

// The two sides of the sort's ping-pong, its per-tile digit counts
// (256 * tiles words) and the 256 digit totals.  `kin` may be key_b.
struct SortBuffers {
  uint64_t *key_a, *key_b;
  uint32_t *pos_a, *pos_b;
  uint32_t *counts, *dtotal;
};

// the n keys `kin` stably sorted on the digits that `differ` names; the
// payload of the sorted pairs is their place in `kin`
inline int enqueue_radix_sort(const uint64_t* kin, uint32_t n, uint64_t differ,
                              const SortBuffers& b, const uint64_t** skey,
                              const uint32_t** spos, hipStream_t s) {
  const uint32_t ntiles = blocks_of(n, kSortTile);
  const uint32_t* pin = nullptr;
  uint64_t* kout = b.key_a;
  uint32_t* pout = b.pos_a;
  bool any = false;
  for (int d = 0; d < 8; ++d) {
    if (((differ >> (8 * d)) & 255u) == 0) continue;  // the same digit in every key
    LAUNCH(sort_count_kernel, ntiles, s, kin, n, 8 * d, b.counts, ntiles);
    LAUNCH(row_scan_kernel, 256, s, b.counts, ntiles, b.dtotal);
    LAUNCH(sort_scatter_kernel, ntiles, s, kin, pin, kout, pout, n, 8 * d, b.counts, b.dtotal,
           ntiles);
    kin = kout;
    pin = pout;
    const bool to_b = kout == b.key_a;
    kout = to_b ? b.key_b : b.key_a;
    pout = to_b ? b.pos_b : b.pos_a;
    any = true;
  }
  if (!any) {
    LAUNCH(sort_identity_kernel, blocks_of(n, 256), s, kin, kout, pout, n);
    pin = pout;
    kin = kout;
  }
  *skey = kin;
  *spos = pin;
  return launched("sort");
}

}  // namespace
}  // namespace psg
