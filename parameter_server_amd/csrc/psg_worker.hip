// psg_worker.hip -- the worker step of the reference's online solver,
// FTRL::updateModel (src/linear_method/ftrl.cc:88-151), on one minibatch
// resident in HBM: Localizer::countUniqIndex and remapIndex
// (src/base/localizer.h:50-87, 110-168), FTRL::countKeys (ftrl.cc:154-174),
// Xw = Z * w (src/base/sparse_matrix.h:73-86), LogitLoss::evaluate / compute
// (src/linear_method/loss.h:73-85) and grad = Z' * (-y tau)
// (base/matrix.h:57-58 over sparse_matrix.h:87-105).  Kernels first, the
// psg_mb_* entry points of include/psg.h after them.
// The kernels of (a), the flag scans of (b), (c), the binary search and the
// ballot fold of (d) are in psg_sort.h, with the sort's shape constants;
// psg_auc.hip includes it too, and psg_blocks.h, the base of both handles.
//
// (a) Sort.  countUniqIndex sorts (key, position) pairs by key
// (parallelSort over pair_).  Here: a stable LSD radix sort of the 64-bit
// keys, 8 bits per pass, the position as a 32-bit payload.  One OR / AND
// reduction over the keys (at load) tells which of the eight digits differ
// between any two keys; a digit that is the same in every key is not sorted
// on.  A pass is three launches: per-tile digit counts (digit-major), one
// workgroup per digit scanning its row of tile counts, and the scatter.  A
// tile is 2048 consecutive pairs; wave w of the workgroup owns the w-th
// quarter of it and walks it 64 pairs at a time, so "earlier in the input"
// is "(wave, step, lane) smaller".  A pair's place among the equal digits of
// its step comes from eight ballots (the lanes that agree on every bit of
// the digit), its place among the wave's earlier steps from a per-wave LDS
// counter that the last lane of each group of equal digits advances, and
// the waves' counters are prefixed across the workgroup: no atomics, and
// the order of equal keys is the input order.  Stability is what makes the
// sorted positions the transpose (CSC) of the minibatch: inside a key's run
// they ascend, that is row after row and in the row's own order.
//
// (b) Run heads of the sorted keys, counted per tile, scanned, then emitted:
// uniq_key, run_start, and run_of (the run of every sorted pair).
// (c) One binary search of the dictionary per run; every pair then takes its
// run's rank + 1 (0: dropped) to its position; a second count / scan / emit
// over the positions compacts the survivors into Z in row order.
// (d) One lane per sorted pair; neighbours of one run fold their counts with
// ballots and one lane adds them to the key's counters (integer atomics).
// (e) times: one lane per row of Z.  trans_times: the term of every sorted
// pair first (all the gathers, in parallel), then one lane per dictionary key
// adds its run's terms in order; a run longer than kLongRun is taken by a
// whole wave instead (the long runs are listed at localize): 64 terms per
// load, several loads ahead, laid out in LDS and added one after the other
// into one accumulator, so the add chain is the reference's and only the
// loads are parallel.  No float atomics, no tree.
// (f) tau, c = -y tau and loss per row as loss.h:74,81 writes them; objv by
// a tree inside each workgroup of 256 rows and a second, single workgroup
// over the partials: the order depends on `rows` alone.
//
// (g) The worker half of the batch solver, Darling::updateModel
// (src/linear_method/darling.cc:196-250), on the same localized minibatch:
// column k of the column-major matrix Darling reads is dictionary key k's
// run of sorted pairs.  computeGradients (:306-356): the two terms of every
// sorted pair of the block (one contiguous range of the pairs), then the
// ordered sums as in (e), both accumulators on one chain.  updateDual
// (:358-435): the per-column state, the factor of every sorted pair of the
// block (all the exp calls, fully parallel), then one lane per row, which
// multiplies its factors in ascending sorted-pair index: a row's entries
// ordered by (column, position) are ordered by sorted-pair index.  The rows'
// lists are built once, at psg_mb_darling_init: the surviving sorted pairs
// stably sorted by row with the passes of (a).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/psg.h"
#include "psg_blocks.h"
#include "psg_device.h"
#include "psg_host.h"
#include "psg_internal.h"
#include "psg_minibatch.h"
#include "psg_sort.h"

namespace psg {
namespace {

#ifndef PSG_LONG_RUN
#define PSG_LONG_RUN 32  // A/B builds: 8, 256
#endif
constexpr uint32_t kLongGrid = 1024;             // workgroups (of 4 waves) over the long runs
constexpr uint32_t kLongRun = PSG_LONG_RUN;      // runs longer than this go to the whole wave

struct KeptFlag {  // position i survives the dictionary
  const uint32_t* remapped;
  __device__ bool operator()(uint32_t i) const { return remapped[i] != 0; }
};

struct KeptEmit {  // ex: survivors before position i
  const uint32_t* remapped;
  const double* value;  // null: binary
  uint32_t* before;     // [n + 1]
  uint32_t* new_index;
  double* new_value;
  __device__ void operator()(uint32_t i, uint32_t ex, bool kept, uint32_t n) const {
    before[i] = ex;
    if (kept) {
      new_index[ex] = remapped[i] - 1;
      if (value) new_value[ex] = value[i];
    }
    if (i == n - 1) before[n] = ex + (kept ? 1u : 0u);
  }
};

__global__ __launch_bounds__(256) void key_cnt_kernel(const uint32_t* __restrict__ run_start,
                                                      uint32_t n_uniq,
                                                      uint32_t* __restrict__ key_cnt) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r < n_uniq) key_cnt[r] = run_start[r + 1] - run_start[r];
}

// the row of every position: offset[row] <= i < offset[row + 1]
__global__ __launch_bounds__(256) void row_of_kernel(const uint64_t* __restrict__ offset,
                                                     uint32_t rows, uint32_t n,
                                                     uint32_t* __restrict__ row_of) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t lo = 0, hi = rows;  // the last row in [lo, hi) with offset[row] <= i
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (offset[mid] <= i) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  row_of[i] = lo;
}

// ---- (c) --------------------------------------------------------------------
__global__ __launch_bounds__(256) void dict_check_kernel(const uint64_t* __restrict__ dict,
                                                         uint32_t ndict,
                                                         unsigned long long* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x + 1;
  if (i < ndict && dict[i - 1] >= dict[i]) atomicAdd(bad, 1ull);
}

// run r: rank + 1 of its key in the dictionary (0: absent), and the run of
// every dictionary key that has one (dict_run preset to all ones: none)
__global__ __launch_bounds__(256) void run_search_kernel(const uint64_t* __restrict__ uniq_key,
                                                         uint32_t n_uniq,
                                                         const uint64_t* __restrict__ dict,
                                                         uint32_t ndict,
                                                         uint32_t* __restrict__ run_rank,
                                                         uint32_t* __restrict__ dict_run) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= n_uniq) return;
  const uint64_t key = uniq_key[r];
  const uint32_t lo = lower_bound(dict, ndict, key);
  const bool found = lo < ndict && dict[lo] == key;
  run_rank[r] = found ? lo + 1 : 0u;
  if (found) dict_run[lo] = (uint32_t)r;
}

// remapped[position] = rank + 1 of the pair's run (localizer.h:123-136)
__global__ __launch_bounds__(256) void remap_kernel(const uint32_t* __restrict__ spos,
                                                    const uint32_t* __restrict__ run_of,
                                                    const uint32_t* __restrict__ run_rank,
                                                    uint32_t n, uint32_t n_uniq,
                                                    uint32_t* __restrict__ remapped) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = run_of[i], p = spos[i];
  if (r < n_uniq && p < n) remapped[p] = run_rank[r];
}

__global__ __launch_bounds__(256) void new_offset_kernel(const uint64_t* __restrict__ offset,
                                                         const uint32_t* __restrict__ before,
                                                         uint32_t rows,
                                                         uint64_t* __restrict__ new_offset) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r <= rows) new_offset[r] = before[offset[r]];
}

// ---- (d), (e) -----------------------------------------------------------------
// the run [*b, *e) of sorted pairs of dictionary key k (empty: none)
__device__ __forceinline__ void run_of_key(uint64_t k, uint32_t ndict,
                                           const uint32_t* __restrict__ dict_run,
                                           const uint32_t* __restrict__ run_start,
                                           uint32_t n_uniq, uint32_t n, uint32_t* b,
                                           uint32_t* e) {
  *b = *e = 0;
  if (k < ndict) {
    const uint32_t r = dict_run[k];
    if (r < n_uniq) {  // all ones (no run) fails this
      const uint32_t hi = run_start[r + 1] < n ? run_start[r + 1] : n;
      *e = hi;
      *b = run_start[r] < hi ? run_start[r] : hi;
    }
  }
}

// the row of sorted pair i (a position past the minibatch, which a correct
// sort never yields, reads row 0 instead of memory it does not own)
__device__ __forceinline__ uint32_t pair_row(const uint32_t* __restrict__ spos,
                                             const uint32_t* __restrict__ row_of, uint64_t i,
                                             uint32_t n, uint32_t* p) {
  *p = spos[i];
  if (*p >= n) *p = 0;
  return row_of[*p];
}

// countKeys (ftrl.cc:164-173): y > 0 is positive, everything else negative.
// One lane per sorted pair; the lanes of a wave that share a run (they are
// neighbours: the pairs are sorted) fold their two counts with ballots, and
// the first lane of each such group adds them to its key's counters (integer
// atomics: exact in any order).  pos / neg zeroed before.
__global__ __launch_bounds__(256) void count_keys_kernel(
    const uint32_t* __restrict__ spos, const uint32_t* __restrict__ row_of,
    const double* __restrict__ y, const uint32_t* __restrict__ run_of,
    const uint32_t* __restrict__ run_rank, uint32_t n, uint32_t n_uniq, uint32_t ndict,
    uint32_t* __restrict__ pos, uint32_t* __restrict__ neg) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool valid = i < n;
  const uint32_t r = valid ? run_of[i] : 0xffffffffu;
  bool positive = false;
  if (valid) {
    uint32_t at;
    positive = y[pair_row(spos, row_of, i, n, &at)] > 0;
  }
  uint32_t cp, cn;
  if (run_label_counts(r, valid, positive, lane, &cp, &cn)) {
    const uint32_t rank = r < n_uniq ? run_rank[r] : 0u;
    if (rank != 0 && rank <= ndict) {
      if (cp) atomicAdd(&pos[rank - 1], cp);
      if (cn) atomicAdd(&neg[rank - 1], cn);
    }
  }
}

// the dictionary keys whose runs are longer than kLongRun, in no particular
// order (what each gives does not depend on it): one wave each in (e)
__global__ __launch_bounds__(256) void long_runs_kernel(
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, uint32_t* __restrict__ long_list, uint32_t* __restrict__ count) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t b, e;
  run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
  if (e - b > kLongRun) {
    const uint32_t at = atomicAdd(count, 1u);
    if (at < ndict) long_list[at] = (uint32_t)k;
  }
}

// times, row-major (sparse_matrix.h:75-86): one lane per row of Z
__global__ __launch_bounds__(256) void times_kernel(const uint64_t* __restrict__ new_offset,
                                                    const uint32_t* __restrict__ new_index,
                                                    const double* __restrict__ new_value,
                                                    uint32_t rows, const double* __restrict__ x,
                                                    double* __restrict__ xw) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= rows) return;
  const uint64_t b = new_offset[i], e = new_offset[i + 1];
  double acc = 0.0;
  if (new_value) {
    for (uint64_t j = b; j < e; ++j) acc = acc + x[new_index[j]] * new_value[j];
  } else {
    for (uint64_t j = b; j < e; ++j) acc = acc + x[new_index[j]];
  }
  xw[i] = acc;  // an empty row: +0.0 (the reference leaves it unwritten, :76)
}

// transTimes (sparse_matrix.h:88-104 on the transpose): g[k] over key k's run
// in ascending position.  Three launches: the term of every sorted pair (all
// the gathers, fully parallel), then the ordered sums over the terms, which
// now lie in run order: one lane per key for runs up to kLongRun, one wave
// per key for the longer ones.
__global__ __launch_bounds__(256) void terms_kernel(const uint32_t* __restrict__ spos,
                                                    const uint32_t* __restrict__ row_of,
                                                    const double* __restrict__ value,
                                                    const double* __restrict__ c, uint32_t n,
                                                    double* __restrict__ term) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t p;
  const uint32_t row = pair_row(spos, row_of, i, n, &p);
  term[i] = value ? c[row] * value[p] : c[row];
}

__global__ __launch_bounds__(256) void trans_times_short_kernel(
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, const double* __restrict__ term, double* __restrict__ g) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= ndict) return;
  uint32_t b, e;
  run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
  if (e - b > kLongRun) return;  // trans_times_long_kernel's
  double acc = 0.0;
  for (uint32_t i = b; i < e; ++i) acc = acc + term[i];
  g[k] = acc;
}

// ((0 + t[lb]) + t[lb + 1]) + ... + t[le - 1], the same in every lane: the
// wave loads kChainAhead x 64 terms ahead of the ones it is adding, lays the
// current ones out in its LDS block `stage` and adds them from there one
// after the other into one accumulator (every lane reads the same word: a
// broadcast).  Reading them out of the lanes' registers instead costs twice
// the time.  LDS operations of one wave run in order; the
// fences keep the compiler from moving the reads across the writes.
#ifndef PSG_CHAIN_AHEAD
#define PSG_CHAIN_AHEAD 8  // A/B builds: 1, 4
#endif
constexpr int kChainAhead = PSG_CHAIN_AHEAD;
__device__ __forceinline__ double chain_sum(const double* __restrict__ term, uint32_t lb,
                                            uint32_t le, uint32_t lane,
                                            double* stage) {
  double a = 0.0, cur[kChainAhead], nxt[kChainAhead];
#pragma unroll
  for (int u = 0; u < kChainAhead; ++u) {
    const uint64_t i = (uint64_t)lb + (uint64_t)u * 64u + lane;
    cur[u] = i < le ? term[i] : 0.0;
    nxt[u] = 0.0;
  }
  for (uint64_t base = lb; base < le; base += 64u * kChainAhead) {
    const uint64_t ahead = base + 64u * kChainAhead;
    if (ahead < le) {
#pragma unroll
      for (int u = 0; u < kChainAhead; ++u) {
        const uint64_t i = ahead + (uint64_t)u * 64u + lane;
        nxt[u] = i < le ? term[i] : 0.0;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < kChainAhead; ++u) stage[u * 64 + lane] = cur[u];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (le - base >= 64u * kChainAhead) {
#pragma unroll 64
      for (int j = 0; j < 64 * kChainAhead; ++j) a = a + stage[j];
    } else {
      const int cnt = (int)(le - base);
      for (int j = 0; j < cnt; ++j) a = a + stage[j];
    }
#pragma unroll
    for (int u = 0; u < kChainAhead; ++u) cur[u] = nxt[u];
  }
  return a;
}

// wave w of the launch takes long_list[w], [w + waves], ...
__global__ __launch_bounds__(256) void trans_times_long_kernel(
    const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ count,
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, const double* __restrict__ term, double* __restrict__ g) {
  __shared__ double stage[4][64 * kChainAhead];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), waves = gridDim.x * 4u;
  const uint32_t nl = *count < ndict ? *count : ndict;
  for (uint32_t j = wave; j < nl; j += waves) {
    const uint32_t k = long_list[j];
    uint32_t b, e;
    run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
    const double a = chain_sum(term, b, e, lane, stage[threadIdx.x >> 6]);
    if (lane == 0 && k < ndict) g[k] = a;
  }
}

// ---- (f) ------------------------------------------------------------------------
using dev::block_tree_sum;  // the fixed-order sum of the workgroup's 256 values

// loss.h:74,81 as written; partial[workgroup] = the tree sum of its 256 losses
__global__ __launch_bounds__(256) void logit_kernel(const double* __restrict__ y,
                                                    const double* __restrict__ xw, uint32_t rows,
                                                    double* __restrict__ tau,
                                                    double* __restrict__ c,
                                                    double* __restrict__ loss,
                                                    double* __restrict__ partial) {
  __shared__ double s[256];
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  double l = 0.0;
  if (i < rows) {
    const double yi = y[i], x = xw[i];
    const double t = 1 / (1 + exp(yi * x));
    l = log(1 + exp(-yi * x));
    tau[i] = t;
    c[i] = -yi * t;
    loss[i] = l;
  }
  block_tree_sum(l, s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}

// lane t adds partials t, t + 256, ... one after the other; then the tree
__global__ __launch_bounds__(256) void objv_kernel(const double* __restrict__ partial,
                                                   uint32_t nparts, double* __restrict__ objv) {
  __shared__ double s[256];
  double a = 0.0;
  for (uint32_t p = threadIdx.x; p < nparts; p += 256) a += partial[p];
  block_tree_sum(a, s);
  if (threadIdx.x == 0) *objv = s[0];
}

// ---- (g) ------------------------------------------------------------------------
using dev::std_min;  // std::min as <algorithm> defines it, not fmin

__device__ __forceinline__ double inactive_value() {  // kInactiveValue_, darling.cc:13-15
  return __longlong_as_double(-1ll);
}

// the dictionary key (column) of sorted pair i; false: dropped by the dictionary
__device__ __forceinline__ bool pair_key(const uint32_t* __restrict__ run_of,
                                         const uint32_t* __restrict__ run_rank, uint64_t i,
                                         uint32_t n_uniq, uint32_t ndict, uint32_t* k) {
  const uint32_t r = run_of[i];
  const uint32_t rank = r < n_uniq ? run_rank[r] : 0u;
  *k = rank - 1;
  return rank != 0 && rank <= ndict;
}

__global__ __launch_bounds__(256) void fill_kernel(double* __restrict__ p, uint32_t n, double v) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) p[i] = v;
}

// dual = exp(y .* Xw), darling.cc:110; dual holds Xw on entry
__global__ __launch_bounds__(256) void dual_init_kernel(const double* __restrict__ y,
                                                        uint32_t rows, double* __restrict__ dual) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < rows) dual[i] = exp(y[i] * dual[i]);
}

// the sort key of sorted pair i for the rows' lists: its row, or `rows` (past
// every row) for a pair the dictionary dropped
__global__ __launch_bounds__(256) void row_key_kernel(
    const uint32_t* __restrict__ spos, const uint32_t* __restrict__ row_of,
    const uint32_t* __restrict__ run_of, const uint32_t* __restrict__ run_rank, uint32_t n,
    uint32_t n_uniq, uint32_t ndict, uint32_t rows, uint64_t* __restrict__ rkey) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t k, p;
  const uint32_t row = pair_row(spos, row_of, i, n, &p);
  rkey[i] = pair_key(run_of, run_rank, i, n_uniq, ndict, &k) && row < rows ? row : rows;
}

// row_start[r] = the first place of the sorted row keys that holds r or more,
// r = 0 .. rows: row r's list is [row_start[r], row_start[r + 1])
__global__ __launch_bounds__(256) void row_start_kernel(const uint64_t* __restrict__ rkey,
                                                        uint32_t n, uint32_t rows,
                                                        uint32_t* __restrict__ row_start) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r > rows) return;
  row_start[r] = lower_bound(rkey, n, r);
}

// range[2k], range[2k + 1] = key k's run of sorted pairs (0, 0: none)
__global__ __launch_bounds__(256) void col_range_kernel(
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, uint32_t* __restrict__ range) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= ndict) return;
  uint32_t b, e;
  run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
  range[2 * k] = b;
  range[2 * k + 1] = e;
}

// binary matrix: d = exp(delta[k]) once per column (darling.cc:338)
__global__ __launch_bounds__(256) void exp_delta_kernel(const double* __restrict__ delta,
                                                        const uint8_t* __restrict__ active,
                                                        uint32_t cb, uint32_t ce,
                                                        double* __restrict__ expd) {
  const uint64_t k = (uint64_t)cb + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k < ce && active[k]) expd[k] = exp(delta[k]);
}

// darling.cc:341-351 for the sorted pairs [lo, hi): term[i] = (-(y tau [v]),
// the term of u): g -= t is g += -t, bit for bit, and the two terms of a pair
// lie side by side so that the sums load them as one.  d: exp(delta) for a
// binary matrix, delta otherwise.  A dropped pair or one of an inactive
// column writes nothing, and nothing reads its terms.
template <bool kBinary>
__global__ __launch_bounds__(256) void darling_terms_kernel(
    const uint32_t* __restrict__ spos, const uint32_t* __restrict__ row_of,
    const uint32_t* __restrict__ run_of, const uint32_t* __restrict__ run_rank,
    const double* __restrict__ value, const double* __restrict__ y,
    const double* __restrict__ dual, const double* __restrict__ d,
    const uint8_t* __restrict__ active, uint32_t lo, uint32_t hi, uint32_t n, uint32_t n_uniq,
    uint32_t ndict, double2* __restrict__ term) {
  const uint64_t i = (uint64_t)lo + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= hi || i >= n) return;
  uint32_t k, p;
  if (!pair_key(run_of, run_rank, i, n_uniq, ndict, &k) || !active[k]) return;
  const uint32_t row = pair_row(spos, row_of, i, n, &p);
  const double tau = 1 / (1 + dual[row]);
  if (kBinary) {
    term[i] = make_double2(-(y[row] * tau), std_min(tau * (1 - tau) * d[k], .25));
  } else {
    const double v = value[p];
    term[i] = make_double2(-(y[row] * tau * v),
                           std_min(tau * (1 - tau) * exp(fabs(v) * d[k]), .25) * v * v);
  }
}

// columns [cb, ce): G and U of a run up to kLongRun, of an empty or absent
// column (+0.0) and of an inactive one (darling.cc:331-336)
__global__ __launch_bounds__(256) void darling_sum_short_kernel(
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, const uint8_t* __restrict__ active, uint32_t cb, uint32_t ce,
    const double2* __restrict__ term, double* __restrict__ g, double* __restrict__ u) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t k = (uint64_t)cb + j;
  if (k >= ce || k >= ndict) return;
  if (!active[k]) {
    g[j] = u[j] = inactive_value();
    return;
  }
  uint32_t b, e;
  run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
  if (e - b > kLongRun) return;  // darling_sum_long_kernel's
  double ag = 0.0, au = 0.0;
  for (uint32_t i = b; i < e; ++i) {
    const double2 t = term[i];
    ag = ag + t.x;
    au = au + t.y;
  }
  g[j] = ag;
  u[j] = au;
}

// chain_sum over pairs of terms: one load and one LDS read bring both terms
// of a sorted pair, and each has its own accumulator, so the two add chains
// overlap.  A load is 16 B per lane here, so half as many are kept ahead.
// stage: 64 x kChainAhead2 double2 of the wave.  Not chain_sum as a template
// over double / double2: its double2 arrays spill (darling_sum_long_kernel 87
// VGPRs and 160 B of scratch per lane, against 117 and none split by hand).
#ifndef PSG_CHAIN_AHEAD2
#define PSG_CHAIN_AHEAD2 4
#endif
constexpr int kChainAhead2 = PSG_CHAIN_AHEAD2;
__device__ __forceinline__ double2 chain_sum2(const double2* __restrict__ term, uint32_t lb,
                                              uint32_t le, uint32_t lane, double2* stage) {
  constexpr int kSpan = 64 * kChainAhead2;
  const double2 zero = make_double2(0.0, 0.0);
  double a0 = 0.0, a1 = 0.0;
  double c0[kChainAhead2], c1[kChainAhead2], n0[kChainAhead2], n1[kChainAhead2];
#pragma unroll
  for (int u = 0; u < kChainAhead2; ++u) {
    const uint64_t i = (uint64_t)lb + (uint64_t)u * 64u + lane;
    const double2 t = i < le ? term[i] : zero;
    c0[u] = t.x;
    c1[u] = t.y;
    n0[u] = n1[u] = 0.0;
  }
  for (uint64_t base = lb; base < le; base += kSpan) {
    const uint64_t ahead = base + kSpan;
    if (ahead < le) {
#pragma unroll
      for (int u = 0; u < kChainAhead2; ++u) {
        const uint64_t i = ahead + (uint64_t)u * 64u + lane;
        const double2 t = i < le ? term[i] : zero;
        n0[u] = t.x;
        n1[u] = t.y;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < kChainAhead2; ++u) stage[u * 64 + lane] = make_double2(c0[u], c1[u]);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (le - base >= (uint64_t)kSpan) {
#pragma unroll 32
      for (int j = 0; j < kSpan; ++j) {
        const double2 t = stage[j];
        a0 = a0 + t.x;
        a1 = a1 + t.y;
      }
    } else {
      const int cnt = (int)(le - base);
      for (int j = 0; j < cnt; ++j) {
        const double2 t = stage[j];
        a0 = a0 + t.x;
        a1 = a1 + t.y;
      }
    }
#pragma unroll
    for (int u = 0; u < kChainAhead2; ++u) {
      c0[u] = n0[u];
      c1[u] = n1[u];
    }
  }
  return make_double2(a0, a1);
}

// wave w of the launch takes long_list[w], [w + waves], ... and keeps the
// active keys of [cb, ce): the list is the dictionary's, in no order, so
// every block's launch walks all of it (the host sizes the grid by its
// length: a few entries per wave)
__global__ __launch_bounds__(256) void darling_sum_long_kernel(
    const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ count,
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, const uint8_t* __restrict__ active, uint32_t cb, uint32_t ce,
    const double2* __restrict__ term, double* __restrict__ g, double* __restrict__ u) {
  __shared__ double2 stage[4][64 * kChainAhead2];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), waves = gridDim.x * 4u;
  const uint32_t nl = *count < ndict ? *count : ndict;
  for (uint32_t j = wave; j < nl; j += waves) {
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)long_list[j]);
    if (k < cb || k >= ce || k >= ndict || !active[k]) continue;
    uint32_t b, e;
    run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
    const double2 a = chain_sum2(term, b, e, lane, stage[threadIdx.x >> 6]);
    if (lane == 0) {
      g[k - cb] = a.x;
      u[k - cb] = a.y;
    }
  }
}

// darling.cc:364-378 for columns [cb, ce); new_w[j] is column cb + j's
__global__ __launch_bounds__(256) void darling_state_kernel(
    const double* __restrict__ new_w, uint32_t cb, uint32_t ce, double delta_max,
    double* __restrict__ cur_w, double* __restrict__ delta, uint8_t* __restrict__ active,
    double* __restrict__ delta_w) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t k = (uint64_t)cb + j;
  if (k >= ce) return;
  const double nw = new_w[j];
  if (nw != nw) {  // inactive(nw), darling.h:35
    active[k] = 0;
    cur_w[k] = 0;
    delta_w[k] = 0;
    return;
  }
  const double dw = nw - cur_w[k];
  delta_w[k] = dw;
  delta[k] = std_min(delta_max, 2 * fabs(dw) + .1);  // newDelta, darling.h:31-33
  cur_w[k] = nw;
}

// the factor of every sorted pair in [lo, hi) (darling.cc:432); -1.0, which
// exp never gives, for a pair of a column that contributes nothing (:424)
template <bool kBinary>
__global__ __launch_bounds__(256) void darling_factor_kernel(
    const uint32_t* __restrict__ spos, const uint32_t* __restrict__ row_of,
    const uint32_t* __restrict__ run_of, const uint32_t* __restrict__ run_rank,
    const double* __restrict__ value, const double* __restrict__ y,
    const double* __restrict__ delta_w, const uint8_t* __restrict__ active, uint32_t lo,
    uint32_t hi, uint32_t n, uint32_t n_uniq, uint32_t ndict, double* __restrict__ factor) {
  const uint64_t i = (uint64_t)lo + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= hi || i >= n) return;
  uint32_t k, p;
  if (!pair_key(run_of, run_rank, i, n_uniq, ndict, &k)) return;  // in no row's list
  const double wd = delta_w[k];
  if (wd == 0 || !active[k]) {
    factor[i] = -1.0;
    return;
  }
  const uint32_t row = pair_row(spos, row_of, i, n, &p);
  factor[i] = kBinary ? exp(y[row] * wd) : exp(y[row] * wd * value[p]);
}

// one lane per row: the row's list holds its sorted pairs in ascending
// index; those in [lo, hi) are the block's, and their factors multiply into
// dual[row] in that order.  A row no factor touches is not written.
__global__ __launch_bounds__(256) void darling_rows_kernel(
    const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ row_pair, uint32_t rows,
    uint32_t lo, uint32_t hi, uint32_t n, const double* __restrict__ factor,
    double* __restrict__ dual) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= rows) return;
  const uint32_t e = row_start[r + 1] < n ? row_start[r + 1] : n;
  uint32_t a = row_start[r] < e ? row_start[r] : e;
  a += lower_bound(row_pair + a, e - a, lo);  // the first entry at or past lo
  double d = 0.0;
  bool touched = false;
  for (uint32_t j = a; j < e; ++j) {
    const uint32_t i = row_pair[j];
    if (i >= hi || i >= n) break;
    const double f = factor[i];
    if (f == -1.0) continue;
    if (!touched) d = dual[r];
    touched = true;
    d = d * f;
  }
  if (touched) dual[r] = d;
}

// log(1 + 1 / dual) per row (darling.cc:506); partial as in logit_kernel
__global__ __launch_bounds__(256) void darling_objv_kernel(const double* __restrict__ dual,
                                                           uint32_t rows,
                                                           double* __restrict__ partial) {
  __shared__ double s[256];
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  block_tree_sum(i < rows ? log(1 + 1 / dual[i]) : 0.0, s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}

}  // namespace
}  // namespace psg

// ------------------------------------------------------------------- host --
using psg::fail;

namespace {

using namespace psg;

// the nnz keys `kin` (which may be the key_b block) stably sorted on the
// digits that `differ` names, through the blocks key_a / key_b / pos_a / pos_b
int enqueue_sort_keys(psg_minibatch* mb, const uint64_t* kin, uint64_t differ, int key_a,
                      int key_b, int pos_a, int pos_b, const uint64_t** skey,
                      const uint32_t** spos, hipStream_t s) {
  const SortBuffers b{mb->at<uint64_t>(key_a), mb->at<uint64_t>(key_b), mb->at<uint32_t>(pos_a),
                      mb->at<uint32_t>(pos_b), mb->at<uint32_t>(B_COUNTS), mb->d_dtotal()};
  return enqueue_radix_sort(kin, (uint32_t)mb->nnz, differ, b, skey, spos, s);
}

// (a): the sorted pairs end in mb->skey / mb->spos
int enqueue_sort(psg_minibatch* mb, hipStream_t s) {
  return enqueue_sort_keys(mb, mb->at<uint64_t>(B_INDEX), mb->differ, B_KEY_A, B_KEY_B, B_POS_A,
                           B_POS_B, &mb->skey, &mb->spos, s);
}

size_t elem_size(int what) {
  switch (what) {
    case PSG_MB_SORTED_POS:
    case PSG_MB_KEY_CNT:
    case PSG_MB_NEW_INDEX:
    case PSG_MB_POS:
    case PSG_MB_NEG:
    case PSG_MB_RUN_START:
    case PSG_MB_REMAPPED:
    case PSG_MB_ROW_OF:
      return 4;
    case PSG_MB_DARLING_ACTIVE:
      return 1;
    case PSG_MB_SLOT:
      return 2;
    default:
      return 8;
  }
}

}  // namespace

namespace psg {

void mb_drop_sharing(psg_minibatch* mb) {
  for (psg_minibatch* sh : mb->sharers) {
    sh->dual_owner = nullptr;
    sh->darling = false;
  }
  mb->sharers.clear();
  if (psg_minibatch* o = mb->dual_owner) {
    o->sharers.erase(std::remove(o->sharers.begin(), o->sharers.end(), mb), o->sharers.end());
    mb->dual_owner = nullptr;
  }
}

int mb_load_begin(psg_minibatch* mb, size_t rows, size_t n, bool valued) {
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;  // the previous minibatch's work
  mb->state = S_NEW;
  mb->darling = false;
  mb->xw_own = false;
  mb->has_slots = mb->groups_ok = false;
  mb_drop_sharing(mb);
  const size_t ntiles = blocks_of(n, kSortTile);
  return mb->need_all({
      {B_OFFSET, 8 * (rows + 1)}, {B_Y, 8 * rows}, {B_INDEX, 8 * n},
      {B_VALUE, valued ? 8 * n : 0}, {B_KEY_A, 8 * n}, {B_KEY_B, 8 * n}, {B_POS_A, 4 * n},
      {B_POS_B, 4 * n}, {B_COUNTS, 4 * 256 * ntiles},
      {B_TILE_SUM, 4 * (size_t)blocks_of(n, kFlagTile) + 4}, {B_UNIQ_KEY, 8 * n},
      {B_KEY_CNT, 4 * n}, {B_RUN_START, 4 * (n + 1)}, {B_RUN_OF, 4 * n}, {B_ROW_OF, 4 * n},
      {B_RUN_RANK, 4 * n}, {B_REMAPPED, 4 * n}, {B_BEFORE, 4 * (n + 1)},
      {B_NEW_OFFSET, 8 * (rows + 1)}, {B_NEW_INDEX, 4 * n}, {B_NEW_VALUE, valued ? 8 * n : 0},
      {B_TERM, 8 * n}, {B_XW, 8 * rows}, {B_TAU, 8 * rows}, {B_C, 8 * rows}, {B_LOSS, 8 * rows},
      {B_PARTIAL, 8 * (size_t)blocks_of(rows, 256) + 8}});
}

int mb_load_finish(psg_minibatch* mb, size_t rows, size_t n, bool valued) {
  hipStream_t s = mb->stream;
  mb->h_small[0] = 0;
  mb->h_small[1] = ~0ull;
  mb->h_small[2] = 0;
  HIP_TRY(hipMemcpyAsync(mb->d_small, mb->h_small, 24, hipMemcpyHostToDevice, s));
  if (n) {
    LAUNCH(row_of_kernel, blocks_of(n, 256), s, mb->at<uint64_t>(B_OFFSET), (uint32_t)rows,
           (uint32_t)n, mb->at<uint32_t>(B_ROW_OF));
    const uint32_t grid = std::min<uint32_t>(blocks_of(n, 256), 2048u);
    LAUNCH(key_bits_kernel, grid, s, mb->at<uint64_t>(B_INDEX), (uint32_t)n, mb->d_small);
    if (int rc = launched("minibatch load")) return rc;
  }
  HIP_TRY(hipMemcpyAsync(mb->h_small, mb->d_small, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  mb->differ = n ? mb->h_small[0] ^ mb->h_small[1] : 0;
  mb->rows = rows;
  mb->nnz = n;
  mb->binary = !valued;
  mb->n_uniq = mb->ndict = 0;
  mb->last_s = nullptr;
  mb->state = S_LOADED;
  return PSG_OK;
}

}  // namespace psg

extern "C" {

size_t psg_mb_sort_tile(void) { return kSortTile; }

int psg_mb_create(psg_ctx* ctx, psg_minibatch** out) {
  if (!ctx || !out) return fail(PSG_ERR_ARG, "null argument");
  *out = nullptr;
  int device, dtype;
  hipStream_t stream;
  psg::ctx_info(ctx, &device, &dtype, &stream);
  if (dtype != PSG_F64) return fail(PSG_ERR_ARG, "a minibatch needs a PSG_F64 context");
  HIP_TRY(hipSetDevice(device));
  psg_minibatch* mb = new (std::nothrow) psg_minibatch();
  if (!mb) return fail(PSG_ERR_OOM, "host allocation");
  if (!mb->open(ctx, kSmallBytes)) {
    psg_mb_destroy(mb);
    return fail(PSG_ERR_OOM, "minibatch control blocks");
  }
  *out = mb;
  return PSG_OK;
}

void psg_mb_destroy(psg_minibatch* mb) {
  if (!mb) return;
  psg::mb_drop_sharing(mb);
  mb->close();
  for (hipEvent_t e : mb->tev)
    if (e) (void)hipEventDestroy(e);
  if (mb->h_text) (void)hipHostFree(mb->h_text);
  if (mb->h_slow) (void)hipHostFree(mb->h_slow);
  delete mb;
}

int psg_mb_load(psg_minibatch* mb, const uint64_t* offset, size_t rows, const uint64_t* index,
                const double* value, const double* y) {
  if (!mb || !offset || (rows && !y)) return fail(PSG_ERR_ARG, "null argument");
  if (rows >= 0xffffffffull) return fail(PSG_ERR_SIZE, "%zu rows >= 2^32 - 1", rows);
  const uint64_t nnz = offset[rows];
  if (nnz >= 0xffffffffull)  // CHECK_LT(idx.size(), kuint32max), localizer.h:54
    return fail(PSG_ERR_SIZE, "%llu entries >= 2^32 - 1: positions are uint32",
                (unsigned long long)nnz);
  if (offset[0] != 0) return fail(PSG_ERR_ARG, "offset[0] = %llu", (unsigned long long)offset[0]);
  for (size_t i = 0; i < rows; ++i)
    if (offset[i] > offset[i + 1]) return fail(PSG_ERR_ARG, "offset decreases at row %zu", i);
  if (nnz && !index) return fail(PSG_ERR_ARG, "null index");
  const size_t n = (size_t)nnz;
  if (int rc = psg::mb_load_begin(mb, rows, n, value != nullptr)) return rc;
  hipStream_t s = mb->stream;
  HIP_TRY(hipMemcpyAsync(mb->b[B_OFFSET].p, offset, 8 * (rows + 1), hipMemcpyHostToDevice, s));
  if (rows) HIP_TRY(hipMemcpyAsync(mb->b[B_Y].p, y, 8 * rows, hipMemcpyHostToDevice, s));
  if (n) {
    HIP_TRY(hipMemcpyAsync(mb->b[B_INDEX].p, index, 8 * n, hipMemcpyHostToDevice, s));
    if (value)
      HIP_TRY(hipMemcpyAsync(mb->b[B_VALUE].p, value, 8 * n, hipMemcpyHostToDevice, s));
  }
  return psg::mb_load_finish(mb, rows, n, value != nullptr);  // the host arrays are free on return
}

int psg_mb_uniq(psg_minibatch* mb, const uint64_t** keys_dev, const uint32_t** cnt_dev,
                size_t* n_out) {
  if (!mb || !n_out) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_LOADED) return fail(PSG_ERR_ARG, "psg_mb_uniq before psg_mb_load");
  HIP_TRY(hipSetDevice(mb->device));
  if (mb->state == S_LOADED) {
    hipStream_t s = mb->stream;
    const uint32_t n = (uint32_t)mb->nnz;
    mb->n_uniq = 0;
    if (n) {
      mb->tick(PSG_MB_STAGE_SORT, 0, s);
      if (int rc = enqueue_sort(mb, s)) return rc;
      mb->tick(PSG_MB_STAGE_SORT, 1, s);
      mb->tick(PSG_MB_STAGE_RUNS, 0, s);
      const HeadFlag f{mb->skey};
      const HeadEmit e{mb->skey, mb->at<uint64_t>(B_UNIQ_KEY), mb->at<uint32_t>(B_RUN_START),
                       mb->at<uint32_t>(B_RUN_OF)};
      enqueue_flag_scan(f, e, n, mb->at<uint32_t>(B_TILE_SUM), mb->d_u32(0), s);
      mb->tick(PSG_MB_STAGE_RUNS, 1, s);
      if (int rc = launched("run heads")) return rc;
      HIP_TRY(hipMemcpyAsync(mb->h_small + 4, mb->d_small + 4, 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      mb->n_uniq = (uint32_t)(mb->h_small[4] & 0xffffffffu);
      if (mb->n_uniq == 0 || mb->n_uniq > n)
        return fail(PSG_ERR_DEVICE, "run count %zu of %u pairs", mb->n_uniq, n);
      LAUNCH(key_cnt_kernel, blocks_of(mb->n_uniq, 256), s, mb->at<uint32_t>(B_RUN_START),
             (uint32_t)mb->n_uniq, mb->at<uint32_t>(B_KEY_CNT));
      if (int rc = launched("key counts")) return rc;
      if (int rc = mb->mark(s)) return rc;
    }
    mb->state = S_UNIQ;
  }
  if (keys_dev) *keys_dev = mb->at<uint64_t>(B_UNIQ_KEY);
  if (cnt_dev) *cnt_dev = mb->at<uint32_t>(B_KEY_CNT);
  *n_out = mb->n_uniq;
  return PSG_OK;
}

int psg_mb_localize(psg_minibatch* mb, const uint64_t* dict_dev, size_t ndict,
                    const uint32_t** pos_dev, const uint32_t** neg_dev, void* stream) {
  if (!mb || (ndict && !dict_dev)) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_UNIQ) return fail(PSG_ERR_ARG, "psg_mb_localize before psg_mb_uniq");
  if (ndict >= 0xffffffffull)  // CHECK_LT(idx_dict.size(), kuint32max), localizer.h:115
    return fail(PSG_ERR_SIZE, "dictionary of %zu keys >= 2^32 - 1", ndict);
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->need_all({{B_DICT_RUN, 4 * ndict}, {B_CNT_POS, 4 * ndict},
                             {B_CNT_NEG, 4 * ndict}, {B_GRAD, 8 * ndict},
                             {B_LONG_LIST, 4 * ndict}}))
    return rc;
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  mb->state = S_UNIQ;
  mb->darling = false;
  mb->xw_own = false;
  const uint32_t n = (uint32_t)mb->nnz, nu = (uint32_t)mb->n_uniq, nd = (uint32_t)ndict;
  const uint32_t rows = (uint32_t)mb->rows;
  uint32_t* before = mb->at<uint32_t>(B_BEFORE);
  mb->tick(PSG_MB_STAGE_LOCALIZE, 0, s);
  HIP_TRY(hipMemsetAsync(mb->d_small + 2, 0, 8, s));
  HIP_TRY(hipMemsetAsync(mb->d_u32(1), 0, 4, s));
  if (nd > 1) LAUNCH(dict_check_kernel, blocks_of(nd - 1, 256), s, dict_dev, nd, mb->d_small + 2);
  if (nd) HIP_TRY(hipMemsetAsync(mb->b[B_DICT_RUN].p, 0xff, 4 * (size_t)nd, s));
  if (n) {
    LAUNCH(run_search_kernel, blocks_of(nu, 256), s, mb->at<uint64_t>(B_UNIQ_KEY), nu, dict_dev,
           nd, mb->at<uint32_t>(B_RUN_RANK), mb->at<uint32_t>(B_DICT_RUN));
    HIP_TRY(hipMemsetAsync(mb->b[B_REMAPPED].p, 0, 4 * (size_t)n, s));
    LAUNCH(remap_kernel, blocks_of(n, 256), s, mb->spos, mb->at<uint32_t>(B_RUN_OF),
           mb->at<uint32_t>(B_RUN_RANK), n, nu, mb->at<uint32_t>(B_REMAPPED));
    const KeptFlag f{mb->at<uint32_t>(B_REMAPPED)};
    const KeptEmit e{mb->at<uint32_t>(B_REMAPPED), mb->binary ? nullptr : mb->at<double>(B_VALUE),
                     before, mb->at<uint32_t>(B_NEW_INDEX), mb->at<double>(B_NEW_VALUE)};
    enqueue_flag_scan(f, e, n, mb->at<uint32_t>(B_TILE_SUM), mb->d_u32(1), s);
  } else {
    HIP_TRY(hipMemsetAsync(before, 0, 4, s));
  }
  LAUNCH(new_offset_kernel, blocks_of((uint64_t)rows + 1, 256), s, mb->at<uint64_t>(B_OFFSET),
         before, rows, mb->at<uint64_t>(B_NEW_OFFSET));
  mb->tick(PSG_MB_STAGE_LOCALIZE, 1, s);
  mb->tick(PSG_MB_STAGE_COUNT_KEYS, 0, s);
  HIP_TRY(hipMemsetAsync(mb->d_small + 5, 0, 8, s));
  if (nd) {
    HIP_TRY(hipMemsetAsync(mb->b[B_CNT_POS].p, 0, 4 * (size_t)nd, s));
    HIP_TRY(hipMemsetAsync(mb->b[B_CNT_NEG].p, 0, 4 * (size_t)nd, s));
    if (n) {
      LAUNCH(count_keys_kernel, blocks_of(n, 256), s, mb->spos, mb->at<uint32_t>(B_ROW_OF),
             mb->at<double>(B_Y), mb->at<uint32_t>(B_RUN_OF), mb->at<uint32_t>(B_RUN_RANK), n, nu,
             nd, mb->at<uint32_t>(B_CNT_POS), mb->at<uint32_t>(B_CNT_NEG));
      LAUNCH(long_runs_kernel, blocks_of(nd, 256), s, mb->at<uint32_t>(B_DICT_RUN), nd,
             mb->at<uint32_t>(B_RUN_START), nu, n, mb->at<uint32_t>(B_LONG_LIST),
             (uint32_t*)(mb->d_small + 5));
    }
  }
  mb->tick(PSG_MB_STAGE_COUNT_KEYS, 1, s);
  if (int rc = launched("localize")) return rc;
  if (int rc = mb->mark(s)) return rc;
  mb->ndict = ndict;
  mb->state = S_LOCAL;
  if (pos_dev) *pos_dev = mb->at<uint32_t>(B_CNT_POS);
  if (neg_dev) *neg_dev = mb->at<uint32_t>(B_CNT_NEG);
  return PSG_OK;
}

namespace {

int enqueue_times(psg_minibatch* mb, const double* x, double* xw, hipStream_t s) {
  if (mb->rows)
    LAUNCH(times_kernel, blocks_of(mb->rows, 256), s, mb->at<uint64_t>(B_NEW_OFFSET),
           mb->at<uint32_t>(B_NEW_INDEX), mb->binary ? nullptr : mb->at<double>(B_NEW_VALUE),
           (uint32_t)mb->rows, x, xw);
  return launched("times");
}

int enqueue_trans_times(psg_minibatch* mb, const double* c, double* g, hipStream_t s) {
  const uint32_t n = (uint32_t)mb->nnz, nd = (uint32_t)mb->ndict, nu = (uint32_t)mb->n_uniq;
  if (nd) {
    if (n)
      LAUNCH(terms_kernel, blocks_of(n, 256), s, mb->spos, mb->at<uint32_t>(B_ROW_OF),
             mb->binary ? nullptr : mb->at<double>(B_VALUE), c, n, mb->at<double>(B_TERM));
    LAUNCH(trans_times_short_kernel, blocks_of(nd, 256), s, mb->at<uint32_t>(B_DICT_RUN), nd,
           mb->at<uint32_t>(B_RUN_START), nu, n, mb->at<double>(B_TERM), g);
    if (n)
      LAUNCH(trans_times_long_kernel, std::min<uint32_t>(blocks_of(nd, 4), kLongGrid), s,
             mb->at<uint32_t>(B_LONG_LIST), (const uint32_t*)(mb->d_small + 5),
             mb->at<uint32_t>(B_DICT_RUN), nd, mb->at<uint32_t>(B_RUN_START), nu, n,
             mb->at<double>(B_TERM), g);
  }
  return launched("trans_times");
}

// A dictionary that was not strictly increasing: reported once, and the
// minibatch is back to where psg_mb_localize can be called again.
int report_dict(psg_minibatch* mb, unsigned long long bad) {
  if (!bad) return PSG_OK;
  mb->state = S_UNIQ;
  return fail(PSG_ERR_UNSORTED, "%llu key pairs of the dictionary not strictly increasing", bad);
}

}  // namespace

int psg_mb_times(psg_minibatch* mb, const double* x_dev, double* xw_dev, void* stream) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_LOCAL) return fail(PSG_ERR_ARG, "psg_mb_times before psg_mb_localize");
  if ((mb->ndict && !x_dev) || (mb->rows && !xw_dev)) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  if (int rc = enqueue_times(mb, x_dev, xw_dev, s)) return rc;
  if (xw_dev == mb->at<double>(B_XW)) mb->xw_own = true;
  return mb->mark(s);
}

int psg_mb_labels(psg_minibatch* mb, const double** y_dev, const double** xw_dev) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_LOADED) return fail(PSG_ERR_ARG, "psg_mb_labels before psg_mb_load");
  if (y_dev) *y_dev = mb->at<double>(B_Y);
  if (xw_dev) *xw_dev = mb->at<double>(B_XW);
  return PSG_OK;
}

int psg_mb_trans_times(psg_minibatch* mb, const double* c_dev, double* g_dev, void* stream) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_LOCAL) return fail(PSG_ERR_ARG, "psg_mb_trans_times before psg_mb_localize");
  if ((mb->rows && !c_dev) || (mb->ndict && !g_dev)) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  if (int rc = enqueue_trans_times(mb, c_dev, g_dev, s)) return rc;
  return mb->mark(s);
}

int psg_mb_gradient(psg_minibatch* mb, int loss, const double* w_dev, const double** grad_dev,
                    double* objv, void* stream) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (loss != PSG_LOSS_LOGIT) return fail(PSG_ERR_ARG, "loss %d: only PSG_LOSS_LOGIT is built", loss);
  if (mb->state < S_LOCAL) return fail(PSG_ERR_ARG, "psg_mb_gradient before psg_mb_localize");
  if (mb->ndict && !w_dev) return fail(PSG_ERR_ARG, "null weights");
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  const uint32_t rows = (uint32_t)mb->rows, nparts = blocks_of(rows, 256);
  mb->tick(PSG_MB_STAGE_TIMES, 0, s);
  if (int rc = enqueue_times(mb, w_dev, mb->at<double>(B_XW), s)) return rc;
  mb->tick(PSG_MB_STAGE_TIMES, 1, s);
  mb->tick(PSG_MB_STAGE_LOGIT, 0, s);
  if (rows)
    LAUNCH(logit_kernel, nparts, s, mb->at<double>(B_Y), mb->at<double>(B_XW), rows,
           mb->at<double>(B_TAU), mb->at<double>(B_C), mb->at<double>(B_LOSS),
           mb->at<double>(B_PARTIAL));
  LAUNCH(objv_kernel, 1, s, mb->at<double>(B_PARTIAL), nparts, (double*)(mb->d_small + 3));
  mb->tick(PSG_MB_STAGE_LOGIT, 1, s);
  if (int rc = launched("logit")) return rc;
  mb->tick(PSG_MB_STAGE_TRANS_TIMES, 0, s);
  if (int rc = enqueue_trans_times(mb, mb->at<double>(B_C), mb->at<double>(B_GRAD), s)) return rc;
  mb->tick(PSG_MB_STAGE_TRANS_TIMES, 1, s);
  if (int rc = mb->mark(s)) return rc;
  HIP_TRY(hipMemcpyAsync(mb->h_small + 2, mb->d_small + 2, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (int rc = report_dict(mb, mb->h_small[2])) return rc;
  if (objv) memcpy(objv, mb->h_small + 3, 8);
  if (grad_dev) *grad_dev = mb->at<double>(B_GRAD);
  mb->state = S_GRAD;
  return PSG_OK;
}

int psg_mb_scratch(psg_minibatch* mb, int slot, size_t bytes, void** dev) {
  if (!mb || !dev || slot < 0 || slot > 3) return fail(PSG_ERR_ARG, "bad scratch slot");
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->need(B_SCRATCH0 + slot, bytes ? bytes : 1)) return rc;
  mb->scratch_len[slot] = bytes;
  *dev = mb->b[B_SCRATCH0 + slot].p;
  return PSG_OK;
}

int psg_mb_profile(psg_minibatch* mb, int on) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  if (on)
    for (hipEvent_t& e : mb->tev)
      if (!e) HIP_TRY(hipEventCreate(&e));
  for (bool& b : mb->tset) b = false;
  mb->prof = on != 0;
  return PSG_OK;
}

int psg_mb_stage_ms(psg_minibatch* mb, double* ms) {
  if (!mb || !ms) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;
  for (int st = 0; st < PSG_MB_STAGES; ++st) {
    ms[st] = -1.0;
    if (!mb->tset[2 * st] || !mb->tset[2 * st + 1]) continue;
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, mb->tev[2 * st], mb->tev[2 * st + 1]));
    ms[st] = t;
  }
  return PSG_OK;
}

int psg_mb_stream(psg_minibatch* mb, void** stream) {
  if (!mb || !stream) return fail(PSG_ERR_ARG, "null argument");
  *stream = (void*)mb->stream;
  return PSG_OK;
}

int psg_mb_read(psg_minibatch* mb, int what, void* out, size_t cap_bytes, size_t* n_out) {
  if (!mb || !n_out) return fail(PSG_ERR_ARG, "null argument");
  *n_out = 0;
  int need_state, id;
  size_t n, first = 0;  // first: the element the array starts at in its block
  const size_t kept_unknown = ~(size_t)0;
  switch (what) {
    case PSG_MB_SORTED_KEY: need_state = S_UNIQ; id = -1; n = mb->nnz; break;
    case PSG_MB_SORTED_POS: need_state = S_UNIQ; id = -2; n = mb->nnz; break;
    case PSG_MB_UNIQ_KEY: need_state = S_UNIQ; id = B_UNIQ_KEY; n = mb->n_uniq; break;
    case PSG_MB_KEY_CNT: need_state = S_UNIQ; id = B_KEY_CNT; n = mb->n_uniq; break;
    case PSG_MB_RUN_START: need_state = S_UNIQ; id = B_RUN_START; n = mb->nnz ? mb->n_uniq + 1 : 0; break;
    case PSG_MB_ROW_OF: need_state = S_LOADED; id = B_ROW_OF; n = mb->nnz; break;
    case PSG_MB_OFFSET: need_state = S_LOADED; id = B_OFFSET; n = mb->rows + 1; break;
    case PSG_MB_INDEX: need_state = S_LOADED; id = B_INDEX; n = mb->nnz; break;
    case PSG_MB_VALUE: need_state = S_LOADED; id = B_VALUE; n = mb->binary ? 0 : mb->nnz; break;
    case PSG_MB_Y: need_state = S_LOADED; id = B_Y; n = mb->rows; break;
    case PSG_MB_SLOT:
      if (!mb->has_slots) return fail(PSG_ERR_ARG, "psg_mb_read: no slot ids since the load");
      need_state = S_LOADED; id = B_SLOT; n = mb->nnz; break;
    case PSG_MB_REMAPPED: need_state = S_LOCAL; id = B_REMAPPED; n = mb->nnz; break;
    case PSG_MB_NEW_OFFSET: need_state = S_LOCAL; id = B_NEW_OFFSET; n = mb->rows + 1; break;
    case PSG_MB_NEW_INDEX: need_state = S_LOCAL; id = B_NEW_INDEX; n = kept_unknown; break;
    case PSG_MB_NEW_VALUE: need_state = S_LOCAL; id = B_NEW_VALUE; n = kept_unknown; break;
    case PSG_MB_POS: need_state = S_LOCAL; id = B_CNT_POS; n = mb->ndict; break;
    case PSG_MB_NEG: need_state = S_LOCAL; id = B_CNT_NEG; n = mb->ndict; break;
    case PSG_MB_XW: need_state = mb->xw_own ? S_LOCAL : S_GRAD; id = B_XW; n = mb->rows; break;
    case PSG_MB_TAU: need_state = S_GRAD; id = B_TAU; n = mb->rows; break;
    case PSG_MB_LOSS: need_state = S_GRAD; id = B_LOSS; n = mb->rows; break;
    case PSG_MB_GRAD: need_state = S_GRAD; id = B_GRAD; n = mb->ndict; break;
    case PSG_MB_SCRATCH + 0: case PSG_MB_SCRATCH + 1: case PSG_MB_SCRATCH + 2:
    case PSG_MB_SCRATCH + 3:
      need_state = S_NEW; id = B_SCRATCH0 + (what - PSG_MB_SCRATCH);
      n = mb->scratch_len[what - PSG_MB_SCRATCH] / 8; break;
    case PSG_MB_DARLING_DUAL: need_state = S_LOCAL; id = B_DUAL; n = mb->rows; break;
    case PSG_MB_DARLING_CUR_W: need_state = S_LOCAL; id = B_CUR_W; n = mb->ndict; break;
    case PSG_MB_DARLING_DELTA: need_state = S_LOCAL; id = B_DELTA; n = mb->ndict; break;
    case PSG_MB_DARLING_ACTIVE: need_state = S_LOCAL; id = B_ACTIVE; n = mb->ndict; break;
    case PSG_MB_DARLING_DELTA_W:
      need_state = S_LOCAL; id = B_DELTA_W; n = mb->last_ce - mb->last_cb; first = mb->last_cb;
      break;
    default: return fail(PSG_ERR_ARG, "psg_mb_read: array %d", what);
  }
  if (what >= PSG_MB_DARLING_DUAL && (!mb->darling || (mb->dual_owner && !mb->dual_owner->darling)))
    return fail(PSG_ERR_ARG, "psg_mb_read: array %d before psg_mb_darling_init", what);
  if (mb->state < need_state)
    return fail(PSG_ERR_ARG, "psg_mb_read: array %d is not computed yet", what);
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;
  if (mb->state >= S_LOCAL) {
    HIP_TRY(hipMemcpy(mb->h_small + 2, mb->d_small + 2, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mb->h_small + 4, mb->d_small + 4, 8, hipMemcpyDeviceToHost));
    if (need_state >= S_LOCAL)
      if (int rc = report_dict(mb, mb->h_small[2])) return rc;
    if (n == kept_unknown) {
      n = (size_t)(mb->h_small[4] >> 32);
      if (n > mb->nnz) return fail(PSG_ERR_DEVICE, "%zu survivors of %zu entries", n, mb->nnz);
      if (what == PSG_MB_NEW_VALUE && mb->binary) n = 0;
    }
  }
  *n_out = n;
  const size_t bytes = n * elem_size(what);
  if (bytes > cap_bytes)
    return fail(PSG_ERR_SIZE, "psg_mb_read: array %d holds %zu bytes, room for %zu", what, bytes,
                cap_bytes);
  if (bytes == 0) return PSG_OK;
  if (!out) return fail(PSG_ERR_ARG, "null output");
  const void* src = id == -1 ? (const void*)mb->skey
                             : id == -2 ? (const void*)mb->spos
                                        : id == B_DUAL ? (const void*)mb->dual()
                                                       : (const void*)mb->b[id].p;
  HIP_TRY(hipMemcpy(out, (const char*)src + first * elem_size(what), bytes,
                    hipMemcpyDeviceToHost));
  return PSG_OK;
}

// ---- (g): the Darling worker ------------------------------------------------
namespace {

int darling_ready(psg_minibatch* mb, const char* who) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_LOCAL || !mb->darling)
    return fail(PSG_ERR_ARG, "%s before psg_mb_darling_init", who);
  if (mb->dual_owner && !mb->dual_owner->darling)
    return fail(PSG_ERR_ARG, "%s: the owner of the shared dual has no Darling state", who);
  return PSG_OK;
}

int darling_block(psg_minibatch* mb, size_t cb, size_t ce, const char* who, uint32_t* lo,
                  uint32_t* hi) {
  if (cb > ce || ce > mb->ndict)
    return fail(PSG_ERR_ARG, "%s: columns [%zu, %zu) of %zu", who, cb, ce, mb->ndict);
  *lo = *hi = 0;
  if (cb < ce) {
    *lo = mb->pair_lo[cb];
    *hi = std::max(mb->pair_hi[ce], *lo);
  }
  return PSG_OK;
}

}  // namespace

int psg_mb_darling_init(psg_minibatch* mb, double delta_init, const double* w_dev,
                        void* stream) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_LOCAL) return fail(PSG_ERR_ARG, "psg_mb_darling_init before psg_mb_localize");
  HIP_TRY(hipSetDevice(mb->device));
  mb->darling = false;
  const bool shares = mb->dual_owner != nullptr;
  if (shares && w_dev)
    return fail(PSG_ERR_ARG, "psg_mb_darling_init with weights on a minibatch that shares a dual");
  if (shares && !mb->dual_owner->darling)
    return fail(PSG_ERR_ARG, "psg_mb_darling_init: the owner of the shared dual has no Darling state");
  const size_t rows_z = mb->rows, n_z = mb->nnz, nd_z = mb->ndict;
  if (int rc = mb->need_all({
      {B_DUAL, shares ? 0 : 8 * rows_z}, {B_CUR_W, 8 * nd_z}, {B_DELTA, 8 * nd_z}, {B_ACTIVE, nd_z},
      {B_DELTA_W, 8 * nd_z}, {B_EXP_DELTA, mb->binary ? 8 * nd_z : 0}, {B_TERM2, 16 * n_z},
      {B_RKEY_A, 8 * n_z}, {B_RKEY_B, 8 * n_z}, {B_RPOS_A, 4 * n_z}, {B_RPOS_B, 4 * n_z},
      {B_ROW_START, 4 * (rows_z + 1)}, {B_COL_RANGE, 8 * nd_z}}))
    return rc;
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  const uint32_t n = (uint32_t)n_z, nd = (uint32_t)nd_z, nu = (uint32_t)mb->n_uniq;
  const uint32_t rows = (uint32_t)rows_z;
  double* dual = mb->at<double>(B_DUAL);
  // dual_ = exp(y .* (X w)), darling.cc:110; the worker's copy of w.  A shared
  // dual is the owner's to fill.
  if (rows && !shares) {
    if (w_dev) {
      if (int rc = enqueue_times(mb, w_dev, dual, s)) return rc;
      LAUNCH(dual_init_kernel, blocks_of(rows, 256), s, mb->at<double>(B_Y), rows, dual);
    } else {
      LAUNCH(fill_kernel, blocks_of(rows, 256), s, dual, rows, 1.0);
    }
  }
  if (nd) {
    if (w_dev)
      HIP_TRY(hipMemcpyAsync(mb->b[B_CUR_W].p, w_dev, 8 * nd_z, hipMemcpyDeviceToDevice, s));
    else
      HIP_TRY(hipMemsetAsync(mb->b[B_CUR_W].p, 0, 8 * nd_z, s));
    HIP_TRY(hipMemsetAsync(mb->b[B_DELTA_W].p, 0, 8 * nd_z, s));
    HIP_TRY(hipMemsetAsync(mb->b[B_ACTIVE].p, 1, nd_z, s));  // :114
    LAUNCH(fill_kernel, blocks_of(nd, 256), s, mb->at<double>(B_DELTA), nd, delta_init);  // :116
    LAUNCH(col_range_kernel, blocks_of(nd, 256), s, mb->at<uint32_t>(B_DICT_RUN), nd,
           mb->at<uint32_t>(B_RUN_START), nu, n, mb->at<uint32_t>(B_COL_RANGE));
  }
  // the rows' lists: the sorted pairs, stably sorted by row
  mb->row_pair = nullptr;
  if (n) {
    uint64_t* rkey = mb->at<uint64_t>(B_RKEY_B);
    LAUNCH(row_key_kernel, blocks_of(n, 256), s, mb->spos, mb->at<uint32_t>(B_ROW_OF),
           mb->at<uint32_t>(B_RUN_OF), mb->at<uint32_t>(B_RUN_RANK), n, nu, nd, rows, rkey);
    uint64_t differ = 1;  // the keys are 0 .. rows: the bits up to rows' highest
    while (differ <= rows) differ <<= 1;
    const uint64_t* sorted_row = nullptr;
    if (int rc = enqueue_sort_keys(mb, rkey, differ - 1, B_RKEY_A, B_RKEY_B, B_RPOS_A, B_RPOS_B,
                                   &sorted_row, &mb->row_pair, s))
      return rc;
    LAUNCH(row_start_kernel, blocks_of((uint64_t)rows + 1, 256), s, sorted_row, n, rows,
           mb->at<uint32_t>(B_ROW_START));
  } else {
    HIP_TRY(hipMemsetAsync(mb->b[B_ROW_START].p, 0, 4 * (rows_z + 1), s));
  }
  if (int rc = launched("darling init")) return rc;
  if (int rc = mb->mark(s)) return rc;
  // every block's range of sorted pairs, kept on the host: a block's launches
  // are sized by it
  std::vector<uint32_t> range;
  try {
    range.resize(2 * nd_z);
    mb->pair_lo.resize(nd_z + 1);
    mb->pair_hi.resize(nd_z + 1);
  } catch (const std::bad_alloc&) {
    return fail(PSG_ERR_OOM, "host allocation");
  }
  HIP_TRY(hipMemcpyAsync(mb->h_small + 2, mb->d_small + 2, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(mb->h_small + 5, mb->d_small + 5, 8, hipMemcpyDeviceToHost, s));
  if (nd)
    HIP_TRY(hipMemcpyAsync(range.data(), mb->b[B_COL_RANGE].p, 8 * nd_z, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (int rc = report_dict(mb, mb->h_small[2])) return rc;
  mb->pair_lo[nd_z] = n;
  for (size_t k = nd_z; k-- > 0;)
    mb->pair_lo[k] = range[2 * k] < range[2 * k + 1] ? range[2 * k] : mb->pair_lo[k + 1];
  mb->pair_hi[0] = 0;
  for (size_t k = 0; k < nd_z; ++k)
    mb->pair_hi[k + 1] = range[2 * k] < range[2 * k + 1] ? range[2 * k + 1] : mb->pair_hi[k];
  mb->n_long = std::min<size_t>((uint32_t)(mb->h_small[5] & 0xffffffffu), nd_z);
  mb->last_cb = mb->last_ce = 0;
  mb->darling = true;
  return PSG_OK;
}

int psg_mb_darling_share_dual(psg_minibatch* mb, psg_minibatch* owner) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (owner) {
    if (owner == mb) return fail(PSG_ERR_ARG, "psg_mb_darling_share_dual with itself");
    if (owner->ctx != mb->ctx) return fail(PSG_ERR_ARG, "minibatches of two contexts");
    if (owner->state < S_LOCAL || !owner->darling)
      return fail(PSG_ERR_ARG, "the owner has not had psg_mb_darling_init");
    if (owner->dual_owner) return fail(PSG_ERR_ARG, "the owner shares another minibatch's dual");
    if (!mb->sharers.empty()) return fail(PSG_ERR_ARG, "the minibatch's own dual is shared");
    if (mb->state < S_LOADED || owner->rows != mb->rows)
      return fail(PSG_ERR_ARG, "%zu rows share a dual of %zu rows", mb->rows, owner->rows);
  }
  if (psg_minibatch* o = mb->dual_owner)
    o->sharers.erase(std::remove(o->sharers.begin(), o->sharers.end(), mb), o->sharers.end());
  mb->dual_owner = nullptr;
  mb->darling = false;  // psg_mb_darling_init comes after this call
  if (owner) {
    try {
      owner->sharers.push_back(mb);
    } catch (const std::bad_alloc&) {
      return fail(PSG_ERR_OOM, "host allocation");
    }
    mb->dual_owner = owner;
  }
  return PSG_OK;
}

int psg_mb_darling_reset_active(psg_minibatch* mb, void* stream) {
  if (int rc = darling_ready(mb, "psg_mb_darling_reset_active")) return rc;
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  if (mb->ndict) HIP_TRY(hipMemsetAsync(mb->b[B_ACTIVE].p, 1, mb->ndict, s));
  return mb->mark(s);
}

int psg_mb_darling_gradients(psg_minibatch* mb, size_t cb, size_t ce, double* g_dev,
                             double* u_dev, void* stream) {
  if (int rc = darling_ready(mb, "psg_mb_darling_gradients")) return rc;
  uint32_t lo, hi;
  if (int rc = darling_block(mb, cb, ce, "psg_mb_darling_gradients", &lo, &hi)) return rc;
  if (cb < ce && (!g_dev || !u_dev)) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  if (cb == ce) return mb->mark(s);
  const uint32_t n = (uint32_t)mb->nnz, nd = (uint32_t)mb->ndict, nu = (uint32_t)mb->n_uniq;
  const uint32_t b = (uint32_t)cb, e = (uint32_t)ce;
  const uint8_t* active = mb->at<uint8_t>(B_ACTIVE);
  double2* term = mb->at<double2>(B_TERM2);
  if (mb->binary)
    LAUNCH(exp_delta_kernel, blocks_of(e - b, 256), s, mb->at<double>(B_DELTA), active, b, e,
           mb->at<double>(B_EXP_DELTA));
  if (hi > lo) {
    if (mb->binary)
      LAUNCH(darling_terms_kernel<true>, blocks_of(hi - lo, 256), s, mb->spos,
             mb->at<uint32_t>(B_ROW_OF), mb->at<uint32_t>(B_RUN_OF), mb->at<uint32_t>(B_RUN_RANK),
             (const double*)nullptr, mb->at<double>(B_Y), mb->dual(),
             mb->at<double>(B_EXP_DELTA), active, lo, hi, n, nu, nd, term);
    else
      LAUNCH(darling_terms_kernel<false>, blocks_of(hi - lo, 256), s, mb->spos,
             mb->at<uint32_t>(B_ROW_OF), mb->at<uint32_t>(B_RUN_OF), mb->at<uint32_t>(B_RUN_RANK),
             mb->at<double>(B_VALUE), mb->at<double>(B_Y), mb->dual(),
             mb->at<double>(B_DELTA), active, lo, hi, n, nu, nd, term);
  }
  LAUNCH(darling_sum_short_kernel, blocks_of(e - b, 256), s, mb->at<uint32_t>(B_DICT_RUN), nd,
         mb->at<uint32_t>(B_RUN_START), nu, n, active, b, e, term, g_dev, u_dev);
  if (hi - lo > kLongRun && mb->n_long)
    LAUNCH(darling_sum_long_kernel, std::min<uint32_t>(blocks_of(mb->n_long, 4), kLongGrid), s,
           mb->at<uint32_t>(B_LONG_LIST), (const uint32_t*)(mb->d_small + 5),
           mb->at<uint32_t>(B_DICT_RUN), nd, mb->at<uint32_t>(B_RUN_START), nu, n, active, b, e,
           term, g_dev, u_dev);
  if (int rc = launched("darling gradients")) return rc;
  return mb->mark(s);
}

int psg_mb_darling_update_dual(psg_minibatch* mb, size_t cb, size_t ce, const double* new_w_dev,
                               double delta_max, void* stream) {
  if (int rc = darling_ready(mb, "psg_mb_darling_update_dual")) return rc;
  uint32_t lo, hi;
  if (int rc = darling_block(mb, cb, ce, "psg_mb_darling_update_dual", &lo, &hi)) return rc;
  if (cb < ce && !new_w_dev) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  mb->last_cb = cb;
  mb->last_ce = ce;
  if (cb == ce) return mb->mark(s);
  const uint32_t n = (uint32_t)mb->nnz, nd = (uint32_t)mb->ndict, nu = (uint32_t)mb->n_uniq;
  const uint32_t rows = (uint32_t)mb->rows;
  uint8_t* active = mb->at<uint8_t>(B_ACTIVE);
  double* factor = mb->at<double>(B_TERM);
  LAUNCH(darling_state_kernel, blocks_of(ce - cb, 256), s, new_w_dev, (uint32_t)cb, (uint32_t)ce,
         delta_max, mb->at<double>(B_CUR_W), mb->at<double>(B_DELTA), active,
         mb->at<double>(B_DELTA_W));
  if (hi > lo && rows) {
    if (mb->binary)
      LAUNCH(darling_factor_kernel<true>, blocks_of(hi - lo, 256), s, mb->spos,
             mb->at<uint32_t>(B_ROW_OF), mb->at<uint32_t>(B_RUN_OF), mb->at<uint32_t>(B_RUN_RANK),
             (const double*)nullptr, mb->at<double>(B_Y), mb->at<double>(B_DELTA_W), active, lo,
             hi, n, nu, nd, factor);
    else
      LAUNCH(darling_factor_kernel<false>, blocks_of(hi - lo, 256), s, mb->spos,
             mb->at<uint32_t>(B_ROW_OF), mb->at<uint32_t>(B_RUN_OF), mb->at<uint32_t>(B_RUN_RANK),
             mb->at<double>(B_VALUE), mb->at<double>(B_Y), mb->at<double>(B_DELTA_W), active, lo,
             hi, n, nu, nd, factor);
    LAUNCH(darling_rows_kernel, blocks_of(rows, 256), s, mb->at<uint32_t>(B_ROW_START),
           mb->row_pair, rows, lo, hi, n, factor, mb->dual());
  }
  if (int rc = launched("darling update_dual")) return rc;
  return mb->mark(s);
}

int psg_mb_darling_objv(psg_minibatch* mb, double* objv, void* stream) {
  if (int rc = darling_ready(mb, "psg_mb_darling_objv")) return rc;
  if (!objv) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  const uint32_t rows = (uint32_t)mb->rows, nparts = blocks_of(rows, 256);
  if (rows)
    LAUNCH(darling_objv_kernel, nparts, s, mb->dual(), rows,
           mb->at<double>(B_PARTIAL));
  LAUNCH(objv_kernel, 1, s, mb->at<double>(B_PARTIAL), nparts, (double*)(mb->d_small + 3));
  if (int rc = launched("darling objv")) return rc;
  if (int rc = mb->mark(s)) return rc;
  HIP_TRY(hipMemcpyAsync(mb->h_small + 3, mb->d_small + 3, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  memcpy(objv, mb->h_small + 3, 8);
  return PSG_OK;
}

int psg_mb_darling_set_state(psg_minibatch* mb, const double* dual, const double* cur_w,
                             const double* delta, const uint8_t* active) {
  if (int rc = darling_ready(mb, "psg_mb_darling_set_state")) return rc;
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;
  if (dual && mb->rows)
    HIP_TRY(hipMemcpy(mb->dual(), dual, 8 * mb->rows, hipMemcpyHostToDevice));
  if (cur_w && mb->ndict)
    HIP_TRY(hipMemcpy(mb->b[B_CUR_W].p, cur_w, 8 * mb->ndict, hipMemcpyHostToDevice));
  if (delta && mb->ndict)
    HIP_TRY(hipMemcpy(mb->b[B_DELTA].p, delta, 8 * mb->ndict, hipMemcpyHostToDevice));
  if (active && mb->ndict) {
    for (size_t k = 0; k < mb->ndict; ++k)
      if (active[k] > 1) return fail(PSG_ERR_ARG, "active[%zu] = %u, not 0 or 1", k, active[k]);
    HIP_TRY(hipMemcpy(mb->b[B_ACTIVE].p, active, mb->ndict, hipMemcpyHostToDevice));
  }
  return PSG_OK;
}

}  // extern "C"
