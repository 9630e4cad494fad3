// psg_colsum.hip -- the blocked summation order of the per-key (column) sums,
// PSG_SUM_BLOCKED of include/psg.h, for psg_mb_trans_times / psg_mb_gradient
// (double), psg_mb_darling_gradients (the pair of terms) and the row forms
// (m <= 32 doubles per term).  The terms come from the term kernels of
// psg_worker.hip and psg_worker_rows.hip, laid out in run order; the runs up
// to kLongRun stay with their short kernels, which give the reference's chain
// in both orders.  Only the sums of the longer runs are here.
//
// The order B(t[0 .. L)), every + one IEEE add:
//   L <= 32:   ((+0.0 + t0) + t1) + ...
//   L <= 4096: 64 partials p_j = ((+0.0 + t[j]) + t[j + 64]) + ..., then for
//              d = 32, 16, 8, 4, 2, 1: p_j = p_j + p_{j+d} for j < d; p_0.
//   longer:    q_k = B(t[4096 k .. min(4096 (k + 1), L))), then B(q).
// Segments count from the run's first term, so B depends on the run alone.
//
// One element shape serves all three callers: a term row of m doubles and a
// group of G lanes per row, G the power of two >= m (a double is m = G = 1,
// the Darling pair m = G = 2 with G and U in neighbouring lanes of one
// 512-B load).  A wave covers R = 64 / G consecutive term rows per load
// instruction, which is one contiguous read of R m doubles.  Load step s
// brings rows s R + sub (sub: the lane's group), whose partial is
// (s mod G) R + sub: a lane keeps the G partials p_v, v = c R + sub, in
// registers, and the partial of a load is known at compile time.  Eight
// loads are issued before their eight adds; no address depends on an
// accumulator.  The tree's steps d >= R pair partials of one lane
// (registers), the steps d < R pair lanes d G apart (ds_bpermute).  A lane's
// chain is at most 64 adds per partial.  Padding a short last load with +0.0
// changes nothing: a partial that starts at +0.0 is never -0.0, and x + 0 = x
// for every other x.
//
// Work split.  Runs of 33 .. 4096: one wave per run over the long-run list
// of the localize.  Longer ("huge") runs: one wave per (run, segment) unit.
// huge_list_kernel lists them; one 64-bit atomic add hands a run its place in
// the list and its first unit together, so the units' bases ascend with the
// place and a unit finds its run by a binary search, done once per localize
// (huge_units_kernel) and kept as a table.  Level 1 writes the q of every
// unit to the handle's scratch; level 2 is the same kernel over q, level 3
// (runs past 4096^2) once more over the level-2 results, whose places are
// base / 4096 + place: ascending and disjoint as well.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/psg.h"
#include "psg_blocks.h"
#include "psg_colsum.h"
#include "psg_ftrl_rows.h"
#include "psg_host.h"
#include "psg_internal.h"
#include "psg_minibatch.h"
#include "psg_sort.h"

namespace psg {
namespace {

static_assert(kColSerial == kLongRun, "the short kernels take the runs of the serial rule");
constexpr int kColAhead = 8;  // loads in flight ahead of their adds

struct Runs {  // the runs of the localized minibatch
  const uint32_t* dict_run;
  const uint32_t* run_start;
  uint32_t ndict, n_uniq, n;
};

// the run [*b, *e) of sorted pairs of dictionary key k, clamped as in
// psg_worker.hip
__device__ __forceinline__ void run_of_key(const Runs& r, uint64_t k, uint32_t* b, uint32_t* e) {
  *b = *e = 0;
  if (k < r.ndict) {
    const uint32_t run = r.dict_run[k];
    if (run < r.n_uniq) {
      const uint32_t hi = r.run_start[run + 1] < r.n ? r.run_start[run + 1] : r.n;
      *e = hi;
      *b = r.run_start[run] < hi ? r.run_start[run] : hi;
    }
  }
}

struct Dest {  // where a finished column sum goes (psg_colsum.h, colsum_enqueue)
  double* g;
  double* u;
  uint32_t cb, ce;
  const uint8_t* active;
};

__device__ __forceinline__ bool dest_takes(const Dest& d, uint32_t k) {
  return k >= d.cb && k < d.ce && (!d.active || d.active[k]);
}

__device__ __forceinline__ void dest_write(const Dest& d, uint32_t k, uint32_t m, uint32_t j,
                                           double v) {
  if (d.u)
    (j ? d.u : d.g)[k - d.cb] = v;
  else
    d.g[(uint64_t)k * m + j] = v;
}

struct Huge {  // the huge runs and their units
  const unsigned long long* ctl;  // runs << 32 | level-1 units
  const uint32_t* key;            // [runs] the dictionary key
  const uint32_t* base;           // [runs] the run's first level-1 unit, ascending
  const uint32_t* unit1;          // [level-1 units] the unit's run
  const uint32_t* unit2;          // [level-2 units] the same for base / kColSeg + place
  uint32_t cap_h, cap_q, cap_q2;  // the room of key / base, unit1 / q1, unit2 / q2
};

__device__ __forceinline__ uint32_t segs_of(uint32_t len) { return (len + kColSeg - 1) / kColSeg; }

// B of the len <= kColSeg term rows src[tb .. tb + len) [m], column lane, in
// the lanes below m; every lane of the wave comes here with the same tb, len
template <int G>
__device__ __forceinline__ double wave_block_sum(const double* __restrict__ src, uint32_t m,
                                                 uint64_t tb, uint32_t len, uint32_t lane) {
  constexpr int R = 64 / G;
  constexpr int kTrip = G < kColAhead ? kColAhead : G;  // load steps per trip: whole 64-row chunks
  const uint32_t j = lane & (uint32_t)(G - 1), sub = lane / (uint32_t)G;
  const bool col = j < m;
  const double* __restrict__ p = src + tb * m + j;
  if (len <= kColSerial) {
    double a = 0.0;
    if (col)
      for (uint32_t i = 0; i < len; ++i) a = a + p[(uint64_t)i * m];
    return a;
  }
  double acc[G];
#pragma unroll
  for (int c = 0; c < G; ++c) acc[c] = 0.0;
  const uint32_t steps = (len + R - 1) / R;
  for (uint32_t s0 = 0; s0 < steps; s0 += kTrip) {
#pragma unroll
    for (int c0 = 0; c0 < kTrip; c0 += kColAhead) {
      double v[kColAhead];
#pragma unroll
      for (int x = 0; x < kColAhead; ++x) {
        const uint32_t i = (s0 + (uint32_t)(c0 + x)) * R + sub;
        v[x] = col && i < len ? p[(uint64_t)i * m] : 0.0;
      }
#pragma unroll
      for (int x = 0; x < kColAhead; ++x) acc[(c0 + x) % G] = acc[(c0 + x) % G] + v[x];
    }
  }
#pragma unroll
  for (int dc = G / 2; dc >= 1; dc >>= 1)  // d = dc R: both partials are this lane's
#pragma unroll
    for (int c = 0; c < dc; ++c) acc[c] = acc[c] + acc[c + dc];
  double a = acc[0];
#pragma unroll
  for (int d = R / 2; d >= 1; d >>= 1) a = a + __shfl_down(a, (unsigned)(d * G), 64);
  return a;
}

// wave w of the launch takes long_list[w], [w + waves], ...: the runs of
// kLongRun + 1 .. kColSeg terms, a whole run each
template <int G>
__global__ __launch_bounds__(256) void colsum_long_kernel(const uint32_t* __restrict__ long_list,
                                                          const uint32_t* __restrict__ count,
                                                          Runs r, const double* __restrict__ term,
                                                          uint32_t m, Dest d) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), waves = gridDim.x * 4u;
  const uint32_t nl = *count < r.ndict ? *count : r.ndict;
  for (uint32_t jl = wave; jl < nl; jl += waves) {
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)long_list[jl]);
    if (k >= r.ndict || !dest_takes(d, k)) continue;
    uint32_t b, e;
    run_of_key(r, k, &b, &e);
    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
    if (e - b <= kLongRun || e - b > kColSeg) continue;  // the short kernel's, the units'
    const double a = wave_block_sum<G>(term, m, b, e - b, lane);
    if (lane < m) dest_write(d, k, m, lane, a);
  }
}

// the dictionary keys whose runs are longer than kColSeg, and each one's
// first unit: ctl += 1 << 32 | segments, so place and base ascend together
__global__ __launch_bounds__(256) void huge_list_kernel(Runs r, uint32_t cap_h, uint32_t cap_q,
                                                        unsigned long long* __restrict__ ctl,
                                                        uint32_t* __restrict__ key,
                                                        uint32_t* __restrict__ base) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t b, e;
  run_of_key(r, k, &b, &e);
  if (e - b <= kColSeg) return;
  const uint32_t nseg = segs_of(e - b);
  const unsigned long long old = atomicAdd(ctl, (1ull << 32) | nseg);
  const uint32_t at = (uint32_t)(old >> 32), first = (uint32_t)old;
  if (at < cap_h && (uint64_t)first + nseg <= cap_q) {  // always: the runs are disjoint pieces of n
    key[at] = (uint32_t)k;
    base[at] = first;
  }
}

// unit u of level 1 belongs to the last run whose base is <= u; a unit of
// level 2 to the last run whose base / kColSeg + place is
__global__ __launch_bounds__(256) void huge_units_kernel(Huge h, uint32_t* __restrict__ unit1,
                                                         uint32_t* __restrict__ unit2) {
  const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const unsigned long long ctl = *h.ctl;
  const uint32_t nh = min((uint32_t)(ctl >> 32), h.cap_h), total = min((uint32_t)ctl, h.cap_q);
  if (nh == 0 || u >= total) return;
  uint32_t lo = 0, hi = nh;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (h.base[mid] <= u) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  unit1[u] = lo;
  if (u >= total / kColSeg + nh || u >= h.cap_q2) return;
  lo = 0, hi = nh;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (h.base[mid] / kColSeg + mid <= u) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  unit2[u] = lo;
}

// One level of the huge runs' sums, a unit per wave.  Level 1: segment seg of
// the run's terms to q1[base + seg].  Level 2: segment seg of the run's q1 to
// q2[base / kColSeg + place + seg], or, when it is the only one, to the
// result.  Level 3: the run's q2 (at most 256) to the result.
template <int G>
__global__ __launch_bounds__(256) void colsum_huge_kernel(int level, Runs r, Huge h,
                                                          const double* __restrict__ term,
                                                          double* __restrict__ q1,
                                                          double* __restrict__ q2, uint32_t m,
                                                          Dest d) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), waves = gridDim.x * 4u;
  const unsigned long long ctl = *h.ctl;
  const uint32_t nh = min((uint32_t)(ctl >> 32), h.cap_h), total = min((uint32_t)ctl, h.cap_q);
  const uint32_t units =
      nh == 0 ? 0u : level == 1 ? total : level == 2 ? min(total / kColSeg + nh, h.cap_q2) : nh;
  for (uint32_t u = wave; u < units; u += waves) {
    uint32_t at = level == 1 ? h.unit1[u] : level == 2 ? h.unit2[u] : u;
    at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
    if (at >= nh) continue;
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.key[at]);
    if (k >= r.ndict || !dest_takes(d, k)) continue;
    uint32_t b, e;
    run_of_key(r, k, &b, &e);
    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
    const uint32_t len0 = e - b;
    if (len0 <= kColSeg) continue;
    const uint32_t base1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.base[at]);
    const uint32_t len1 = segs_of(len0), base2 = base1 / kColSeg + at, len2 = segs_of(len1);
    if ((uint64_t)base1 + len1 > h.cap_q || (uint64_t)base2 + len2 > h.cap_q2) continue;  // never
    const double* src;
    double* dst = nullptr;  // null: the result
    uint64_t tb, to = 0;
    uint32_t len;
    if (level == 1) {
      const uint32_t seg = u - base1;
      if (seg >= len1) continue;
      src = term;
      tb = (uint64_t)b + (uint64_t)seg * kColSeg;
      len = min(kColSeg, len0 - seg * kColSeg);
      dst = q1;
      to = (uint64_t)base1 + seg;
    } else if (level == 2) {
      const uint32_t seg = u - base2;
      if (seg >= len2) continue;
      src = q1;
      tb = (uint64_t)base1 + (uint64_t)seg * kColSeg;
      len = min(kColSeg, len1 - seg * kColSeg);
      if (len2 > 1) {
        dst = q2;
        to = (uint64_t)base2 + seg;
      }
    } else {
      if (len2 <= 1) continue;
      src = q2;
      tb = base2;
      len = len2;
    }
    const double a = wave_block_sum<G>(src, m, tb, len, lane);
    if (lane < m) {
      if (dst)
        dst[to * m + lane] = a;
      else
        dest_write(d, k, m, lane, a);
    }
  }
}

// the room of the huge runs' tables for n terms: the runs are disjoint pieces
// of n longer than kColSeg, and a run of L terms has at most L / kColSeg + 1
// segments
struct Caps {
  uint32_t h, q, q2;
};
Caps caps_of(uint64_t n) {
  Caps c;
  c.h = (uint32_t)(n / kColSeg + 1);
  c.q = (uint32_t)(n / kColSeg + c.h + 1);
  c.q2 = c.q / kColSeg + c.h + 1;
  return c;
}

Huge huge_of(const psg_minibatch* mb) {
  const Caps c = caps_of(mb->nnz);
  return Huge{mb->at<unsigned long long>(B_CS_CTL), mb->at<uint32_t>(B_CS_HKEY),
              mb->at<uint32_t>(B_CS_HBASE),         mb->at<uint32_t>(B_CS_UNIT1),
              mb->at<uint32_t>(B_CS_UNIT2),         c.h, c.q, c.q2};
}

Runs runs_of(const psg_minibatch* mb) {
  return Runs{mb->at<uint32_t>(B_DICT_RUN), mb->at<uint32_t>(B_RUN_START), (uint32_t)mb->ndict,
              (uint32_t)mb->n_uniq, (uint32_t)mb->nnz};
}

template <int G>
void launch_sums(psg_minibatch* mb, const double* term, uint32_t m, const Dest& d,
                 uint32_t long_grid, hipStream_t s) {
  const Runs r = runs_of(mb);
  LAUNCH(colsum_long_kernel<G>, long_grid, s, mb->at<uint32_t>(B_LONG_LIST),
         (const uint32_t*)(mb->d_small + 5), r, term, m, d);
  if (mb->nnz <= kColSeg) return;  // no run is longer
  const Huge h = huge_of(mb);
  const int levels = mb->nnz > (uint64_t)kColSeg * kColSeg ? 3 : 2;
  for (int level = 1; level <= levels; ++level) {
    const uint32_t bound = level == 1 ? h.cap_q : level == 2 ? h.cap_q2 : h.cap_h;
    LAUNCH(colsum_huge_kernel<G>, std::min<uint32_t>(blocks_of(bound, 4), kLongGrid), s, level, r,
           h, term, mb->at<double>(B_CS_Q1), mb->at<double>(B_CS_Q2), m, d);
  }
}

}  // namespace

int colsum_prepare(psg_minibatch* mb, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  mb->cs_ready = false;
  if (mb->nnz > kColSeg && mb->ndict) {
    const Caps c = caps_of(mb->nnz);
    if (int rc = mb->need_all({{B_CS_CTL, 8}, {B_CS_HKEY, 4 * (size_t)c.h},
                               {B_CS_HBASE, 4 * (size_t)c.h}, {B_CS_UNIT1, 4 * (size_t)c.q},
                               {B_CS_UNIT2, 4 * (size_t)c.q2}}))
      return rc;
    const Huge h = huge_of(mb);
    HIP_TRY(hipMemsetAsync(mb->b[B_CS_CTL].p, 0, 8, s));
    LAUNCH(huge_list_kernel, blocks_of(mb->ndict, 256), s, runs_of(mb), c.h, c.q,
           mb->at<unsigned long long>(B_CS_CTL), mb->at<uint32_t>(B_CS_HKEY),
           mb->at<uint32_t>(B_CS_HBASE));
    LAUNCH(huge_units_kernel, blocks_of(c.q, 256), s, h, mb->at<uint32_t>(B_CS_UNIT1),
           mb->at<uint32_t>(B_CS_UNIT2));
    if (int rc = launched("blocked sums: unit table")) return rc;
  }
  mb->cs_ready = true;
  return PSG_OK;
}

int colsum_enqueue(psg_minibatch* mb, const double* term, int m, double* g, double* u,
                   uint32_t cb, uint32_t ce, const uint8_t* active, size_t long_bound,
                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!mb->nnz || !mb->ndict || !long_bound) return PSG_OK;
  if (m < 1 || m > PSG_FTRL_MAX_MODELS || (u && m != 2))
    return fail(PSG_ERR_ARG, "blocked sums: %d columns", m);
  if (!mb->cs_ready)
    if (int rc = colsum_prepare(mb, stream)) return rc;
  if (mb->nnz > kColSeg) {  // the partials of the units, level 1 and level 2
    const Caps c = caps_of(mb->nnz);
    if (int rc = mb->need_all({{B_CS_Q1, 8 * (size_t)c.q * m}, {B_CS_Q2, 8 * (size_t)c.q2 * m}}))
      return rc;
  }
  const Dest d{g, u, cb, ce, active};
  const uint32_t grid = std::min<uint32_t>(blocks_of(long_bound, 4), kLongGrid);
  switch (group_shift(m)) {
    case 0: launch_sums<1>(mb, term, (uint32_t)m, d, grid, s); break;
    case 1: launch_sums<2>(mb, term, (uint32_t)m, d, grid, s); break;
    case 2: launch_sums<4>(mb, term, (uint32_t)m, d, grid, s); break;
    case 3: launch_sums<8>(mb, term, (uint32_t)m, d, grid, s); break;
    case 4: launch_sums<16>(mb, term, (uint32_t)m, d, grid, s); break;
    default: launch_sums<32>(mb, term, (uint32_t)m, d, grid, s); break;
  }
  return launched("blocked sums");
}

}  // namespace psg

extern "C" {

int psg_mb_set_sum_order(psg_minibatch* mb, int order) {
  if (!mb) return psg::fail(PSG_ERR_ARG, "null argument");
  if (order != PSG_SUM_REFERENCE && order != PSG_SUM_BLOCKED)
    return psg::fail(PSG_ERR_ARG, "psg_mb_set_sum_order: order %d", order);
  mb->sum_order = order;
  return PSG_OK;
}

int psg_mb_sum_order(psg_minibatch* mb, int* order) {
  if (!mb || !order) return psg::fail(PSG_ERR_ARG, "null argument");
  *order = mb->sum_order;
  return PSG_OK;
}

}  // extern "C"
