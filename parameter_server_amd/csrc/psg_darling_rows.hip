// psg_darling_rows.hip -- the batch solver (Darling, darling.cc:196-267) for m
// models over one resident minibatch: the worker's computeGradients (:306-356),
// updateDual (:358-435), its lines of preprocessData (:110-117) and
// evaluateProgress (:506) as psg_mb_darling_rows_*, and the server's
// updateWeight (:437-477) and progress (:538-555) on plain [n][m] device
// arrays as psg_darling_rows_* (include/psg.h).  A model is a setting (lambda,
// eta, kkt threshold, delta_max); the column runs, the rows' lists, the values
// and the labels are psg_worker.hip's, built once and read by every model.
//
// Column j of every output is bit for bit the scalar kernels' result for
// model j alone (psg_worker.hip (g), psg_darling.hip): the same rounded
// operations in the same order on one accumulator per (key, model) or (row,
// model), the same device exp / log.
//
// Work split (the row forms of psg_worker_rows.hip): a group of G lanes, G the
// power of two >= m, owns one sorted pair, one dictionary key, one row or one
// server position; lane j keeps model j's accumulator.  The pair's position,
// row, value and key words are the same address in every lane of the group
// (one broadcast read); dual, cur_w, delta, the table and the term rows are
// one contiguous read of 8 m or 16 m bytes.  The active set is one uint32 per
// key, bit j for model j: a group reads its key's word once, and a group that
// changes it assembles the new word with one ballot and one shift and stores
// it from one lane.  No atomics on the mask, no float atomics anywhere.
//
// gradients: (1) tau = 1 / (1 + dual) with y tau and tau (1 - tau) once per
// (row, model) into two [rows][m] tables -- a pair of the scalar path
// recomputes them, here the per-pair path has no divide; (2) exp(delta) per
// (column, model) for a binary matrix; (3) the (g, u) term pair of every
// sorted pair of the block, [pair - lo][m] double2, so that scratch grows
// with the block's pairs and not with nnz; (4) the ordered sums: a group per
// key for runs up to kLongRun, a whole wave for a longer run, which streams
// the run's contiguous term rows through LDS and adds each model's two chains
// from there (they overlap, as in chain_sum2).  The table keeps y tau, not
// -(y tau): the sign is flipped where the term is formed, an operand modifier,
// so the valued form -((y tau) v) is the scalar expression operator by
// operator.  The binary g sum reads the term rows like the valued one (the
// gather of table rows inside the ordered sum is not built: DESIGN.md 4.9b).
//
// update_dual: the state kernel over (key, model), the factors of the block's
// pairs ([pair - lo][m], -1.0 = contributes nothing, per model), then a group
// per row multiplying model j's live factors in ascending sorted-pair index.
//
// Server: a group per position; the new mask word by a ballot; the violation
// per model as a max on bit patterns over the workgroup's groups in LDS, one
// atomic max per (workgroup, model) into one of kRowSlots rows of slots, and
// a second kernel that folds the rows into vio[m] and re-zeroes them
// (psg_darling.hip's header says why not one address per model).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/psg.h"
#include "psg_blocks.h"
#include "psg_ctx.h"
#include "psg_device.h"
#include "psg_ftrl_rows.h"
#include "psg_host.h"
#include "psg_internal.h"
#include "psg_minibatch.h"
#include "psg_sort.h"

namespace psg {
namespace {

using dev::std_max;
using dev::std_min;

constexpr int kDrMax = PSG_DARLING_MAX_MODELS;
#ifndef PSG_DROWS_AHEAD
#define PSG_DROWS_AHEAD 4  // loads of 64 double2 a long run's wave keeps ahead of its adds
#endif
constexpr int kAhead = PSG_DROWS_AHEAD;
constexpr int kObjvCols = 8;   // columns per pass of the objv kernel's LDS block
constexpr int kRowSlots = 64;  // rows of kDrMax violation slots (256 B each)

struct PerModel {  // a by-value kernel argument: one double per model
  double v[kDrMax];
};
struct ServerParams {
  double eta[kDrMax], lambda[kDrMax], kkt[kDrMax], delta_max[kDrMax];
};

__device__ __forceinline__ double inactive_value() {  // kInactiveValue_, darling.cc:13-15
  return __longlong_as_double(-1ll);
}

// the bits of `pred` over the lanes of this lane's group, lane j at bit j
__device__ __forceinline__ uint32_t group_ballot(bool pred, uint32_t gs) {
  const unsigned long long b = __ballot(pred);
  const uint32_t base = (threadIdx.x & 63u) & ~((1u << gs) - 1u);
  const uint32_t gmask = gs == 5 ? 0xffffffffu : ((1u << (1u << gs)) - 1u);
  return (uint32_t)(b >> base) & gmask;
}

__device__ __forceinline__ void run_of_key(uint64_t k, uint32_t ndict,
                                           const uint32_t* __restrict__ dict_run,
                                           const uint32_t* __restrict__ run_start,
                                           uint32_t n_uniq, uint32_t n, uint32_t* b, uint32_t* e) {
  *b = *e = 0;
  if (k < ndict) {
    const uint32_t r = dict_run[k];
    if (r < n_uniq) {
      const uint32_t hi = run_start[r + 1] < n ? run_start[r + 1] : n;
      *e = hi;
      *b = run_start[r] < hi ? run_start[r] : hi;
    }
  }
}

struct Pairs {  // the sorted pairs and what they point at (psg_worker.hip's arrays)
  const uint32_t* spos;
  const uint32_t* row_of;
  const uint32_t* run_of;
  const uint32_t* run_rank;
  const double* value;  // null: binary
  const double* y;
  uint32_t n, n_uniq, ndict, rows;
};

// the dictionary key of sorted pair i (false: dropped), its position and row
__device__ __forceinline__ bool pair_at(const Pairs& P, uint64_t i, uint32_t* k, uint32_t* p,
                                        uint32_t* row) {
  const uint32_t r = P.run_of[i];
  const uint32_t rank = r < P.n_uniq ? P.run_rank[r] : 0u;
  *k = rank - 1;
  if (rank == 0 || rank > P.ndict) return false;
  *p = P.spos[i];
  if (*p >= P.n) *p = 0;
  *row = P.row_of[*p];
  if (*row >= P.rows) *row = 0;  // never: rows of the minibatch
  return true;
}

// ---- the rows' lists (model-independent; psg_worker.hip builds the same at
// psg_mb_darling_init, into the same blocks) ----------------------------------
__global__ __launch_bounds__(256) void dr_row_key_kernel(Pairs P, uint64_t* __restrict__ rkey) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n) return;
  uint32_t k, p, row;
  const uint32_t pp = P.spos[i] < P.n ? P.spos[i] : 0u;
  const uint32_t raw_row = P.row_of[pp];
  rkey[i] = pair_at(P, i, &k, &p, &row) && raw_row < P.rows ? raw_row : P.rows;
}

__global__ __launch_bounds__(256) void dr_row_start_kernel(const uint64_t* __restrict__ rkey,
                                                           uint32_t n, uint32_t rows,
                                                           uint32_t* __restrict__ row_start) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r > rows) return;
  row_start[r] = lower_bound(rkey, n, r);
}

__global__ __launch_bounds__(256) void dr_col_range_kernel(
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, uint32_t* __restrict__ range) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= ndict) return;
  uint32_t b, e;
  run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
  range[2 * k] = b;
  range[2 * k + 1] = e;
}

// ---- init ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void dr_fill_kernel(double* __restrict__ p, uint64_t n,
                                                      double v) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ __launch_bounds__(256) void dr_copy_kernel(double* __restrict__ p,
                                                      const double* __restrict__ q, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) p[i] = q[i];
}

// n words = v (the mask words, the row starts of a minibatch with no entry)
__global__ __launch_bounds__(256) void dr_mask_fill_kernel(uint32_t* __restrict__ mask,
                                                           uint32_t ndict, uint32_t all) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k < ndict) mask[k] = all;
}

// dual = exp(y .* Xw), darling.cc:110; dual holds Xw [rows][m] on entry
__global__ __launch_bounds__(256) void dr_dual_init_kernel(const double* __restrict__ y,
                                                           uint32_t rows, uint32_t m,
                                                           double* __restrict__ dual) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < (uint64_t)rows * m) dual[i] = exp(y[i / m] * dual[i]);
}

// ---- gradients ------------------------------------------------------------------
// darling.cc:342 once per (row, model): tau, then y tau and tau (1 - tau)
__global__ __launch_bounds__(256) void dr_table_kernel(const double* __restrict__ y,
                                                       const double* __restrict__ dual,
                                                       uint32_t rows, uint32_t m,
                                                       double* __restrict__ ytau,
                                                       double* __restrict__ q) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (uint64_t)rows * m) return;
  const double tau = 1 / (1 + dual[i]);
  ytau[i] = y[i / m] * tau;
  q[i] = tau * (1 - tau);
}

// binary matrix: exp(delta) once per (column, model) (darling.cc:338)
__global__ __launch_bounds__(256) void dr_exp_delta_kernel(const double* __restrict__ delta,
                                                           const uint32_t* __restrict__ mask,
                                                           uint32_t cb, uint32_t ce, uint32_t m,
                                                           double* __restrict__ expd) {
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t k = cb + e / m;
  const uint32_t j = (uint32_t)(e % m);
  if (k < ce && ((mask[k] >> j) & 1u)) expd[k * m + j] = exp(delta[k * m + j]);
}

// darling.cc:341-351 for the sorted pairs [lo, hi), a group per pair:
// term[pair - lo][j] = (-(y tau [v]), the term of u) of model j.  d: exp(delta)
// for a binary matrix, delta otherwise.  A dropped pair and an inactive (key,
// model) write nothing, and nothing reads their terms.
template <bool kBinary>
__global__ __launch_bounds__(256) void dr_terms_kernel(
    Pairs P, const uint32_t* __restrict__ mask, const double* __restrict__ ytau,
    const double* __restrict__ q, const double* __restrict__ d, uint32_t lo, uint32_t hi,
    uint32_t m, uint32_t gs, double2* __restrict__ term) {
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t t = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  const uint64_t i = (uint64_t)lo + t;
  if (i >= hi || i >= P.n || j >= m) return;
  uint32_t k, p, row;
  if (!pair_at(P, i, &k, &p, &row) || !((mask[k] >> j) & 1u)) return;
  const uint64_t at = (uint64_t)row * m + j;
  const double yt = ytau[at], qq = q[at], dk = d[(uint64_t)k * m + j];
  if (kBinary) {
    term[t * m + j] = make_double2(-yt, std_min(qq * dk, .25));
  } else {
    const double v = P.value[p];
    term[t * m + j] = make_double2(-(yt * v), std_min(qq * exp(fabs(v) * dk), .25) * v * v);
  }
}

// columns [cb, ce), a group per column: G and U of a run up to kLongRun, of an
// empty or absent column (+0.0) and of an inactive (key, model) (:331-336)
__global__ __launch_bounds__(256) void dr_sum_short_kernel(
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, const uint32_t* __restrict__ mask, uint32_t cb, uint32_t ce,
    uint32_t lo, uint32_t hi, const double2* __restrict__ term, uint32_t m, uint32_t gs,
    double* __restrict__ g, double* __restrict__ u) {
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t c = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  const uint64_t k = (uint64_t)cb + c;
  if (k >= ce || k >= ndict || j >= m) return;
  if (!((mask[k] >> j) & 1u)) {
    g[c * m + j] = u[c * m + j] = inactive_value();
    return;
  }
  uint32_t b, e;
  run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
  if (e - b > kLongRun) return;  // dr_sum_long_kernel's
  if (b < lo || e > hi) b = e = lo;  // never: the block's pairs hold its columns' runs
  double ag = 0.0, au = 0.0;
  const double2* tp = term + (uint64_t)(b - lo) * m + j;
  for (uint32_t i = b; i < e; ++i, tp += m) {
    const double2 t = *tp;
    ag = ag + t.x;
    au = au + t.y;
  }
  g[c * m + j] = ag;
  u[c * m + j] = au;
}

// A whole wave per run longer than kLongRun: wave w of the launch takes
// long_list[w], [w + waves], ... and keeps the keys of [cb, ce) with a live
// model.  The run's term rows are one contiguous piece, [e - b][m] double2; the
// wave copies it 64 double2 per load, kAhead loads ahead, into its LDS block
// whole pairs at a time, and lane j < m adds model j's two terms of each pair
// from there, one pair after the other, on its own (g, u) accumulators: two
// independent add chains per lane.  The x and y halves travel in separate
// register arrays (double2 arrays spill: psg_worker.hip, chain_sum2).
__global__ __launch_bounds__(256) void dr_sum_long_kernel(
    const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ count,
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, const uint32_t* __restrict__ mask, uint32_t cb, uint32_t ce,
    uint32_t lo, uint32_t hi, const double2* __restrict__ term, uint32_t m,
    double* __restrict__ g, double* __restrict__ u) {
  __shared__ double2 stage[4][64 * kAhead];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t pps = (64u * kAhead) / m, span = pps * m;  // pairs, double2 per refill
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), waves = gridDim.x * 4u;
  const uint32_t all = m == 32 ? 0xffffffffu : ((1u << m) - 1u);
  double2* st = stage[threadIdx.x >> 6];
  const double2 zero = make_double2(0.0, 0.0);
  const uint32_t nl = *count < ndict ? *count : ndict;
  for (uint32_t jl = wave; jl < nl; jl += waves) {
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)long_list[jl]);
    if (k < cb || k >= ce || k >= ndict) continue;
    const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)mask[k]) & all;
    if (word == 0) continue;
    uint32_t b, e;
    run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    e = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
    if (b < lo || e > hi) continue;  // never
    const uint64_t tb = (uint64_t)(b - lo) * m, te = (uint64_t)(e - lo) * m;
    double a0 = 0.0, a1 = 0.0;
    double cx[kAhead], cy[kAhead], nx[kAhead], ny[kAhead];
#pragma unroll
    for (int w = 0; w < kAhead; ++w) {
      const uint32_t off = (uint32_t)w * 64u + lane;
      const double2 t = off < span && tb + off < te ? term[tb + off] : zero;
      cx[w] = t.x;
      cy[w] = t.y;
      nx[w] = ny[w] = 0.0;
    }
    for (uint64_t base = tb; base < te; base += span) {
      const uint64_t ahead = base + span;
      if (ahead < te) {
#pragma unroll
        for (int w = 0; w < kAhead; ++w) {
          const uint32_t off = (uint32_t)w * 64u + lane;
          const double2 t = off < span && ahead + off < te ? term[ahead + off] : zero;
          nx[w] = t.x;
          ny[w] = t.y;
        }
      }
      // LDS operations of one wave run in order; the fences keep the compiler
      // from moving the reads across the writes (as chain_sum, psg_worker.hip)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int w = 0; w < kAhead; ++w) st[w * 64 + lane] = make_double2(cx[w], cy[w]);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint64_t left = (te - base) / m;
      const uint32_t cnt = left < pps ? (uint32_t)left : pps;
      if (lane < m) {  // four LDS reads in flight ahead of the two add chains
        const double2* col = st + lane;
        uint32_t t = 0;
        for (; t + 4 <= cnt; t += 4, col += 4 * m) {
          double2 v[4];
#pragma unroll
          for (int w = 0; w < 4; ++w) v[w] = col[w * m];
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            a0 = a0 + v[w].x;
            a1 = a1 + v[w].y;
          }
        }
        for (; t < cnt; ++t, col += m) {
          const double2 v = *col;
          a0 = a0 + v.x;
          a1 = a1 + v.y;
        }
      }
#pragma unroll
      for (int w = 0; w < kAhead; ++w) {
        cx[w] = nx[w];
        cy[w] = ny[w];
      }
    }
    if (lane < m && ((word >> lane) & 1u)) {
      g[(uint64_t)(k - cb) * m + lane] = a0;
      u[(uint64_t)(k - cb) * m + lane] = a1;
    }
  }
}

// ---- update_dual ------------------------------------------------------------------
// darling.cc:364-378 for columns [cb, ce), a group per column; new_w[c][j] is
// column cb + c's weight of model j.  The group's cleared bits leave as one
// word from its first lane.
__global__ __launch_bounds__(256) void dr_state_kernel(
    const double* __restrict__ new_w, uint32_t cb, uint32_t ce, uint32_t m, uint32_t gs,
    PerModel delta_max, double* __restrict__ cur_w, double* __restrict__ delta,
    uint32_t* __restrict__ mask, double* __restrict__ delta_w) {
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t c = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  const uint64_t k = (uint64_t)cb + c;
  const bool in = k < ce && j < m;
  bool clear = false;
  if (in) {
    const uint64_t at = k * m + j;
    const double nw = new_w[c * m + j];
    if (nw != nw) {  // inactive(nw), darling.h:35
      clear = true;
      cur_w[at] = 0;
      delta_w[at] = 0;
    } else {
      const double dw = nw - cur_w[at];
      delta_w[at] = dw;
      delta[at] = std_min(delta_max.v[j], 2 * fabs(dw) + .1);  // newDelta, darling.h:31-33
      cur_w[at] = nw;
    }
  }
  const uint32_t off = group_ballot(clear, gs);
  if (j == 0 && k < ce && off) mask[k] = mask[k] & ~off;
}

// the factor of model j of every sorted pair in [lo, hi) (darling.cc:432);
// -1.0, which exp never gives, where the (column, model) contributes nothing
// (:424)
template <bool kBinary>
__global__ __launch_bounds__(256) void dr_factor_kernel(
    Pairs P, const uint32_t* __restrict__ mask, const double* __restrict__ delta_w, uint32_t lo,
    uint32_t hi, uint32_t m, uint32_t gs, double* __restrict__ factor) {
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t t = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  const uint64_t i = (uint64_t)lo + t;
  if (i >= hi || i >= P.n || j >= m) return;
  uint32_t k, p, row;
  if (!pair_at(P, i, &k, &p, &row)) return;  // in no row's list
  const double wd = delta_w[(uint64_t)k * m + j];
  if (wd == 0 || !((mask[k] >> j) & 1u)) {
    factor[t * m + j] = -1.0;
    return;
  }
  factor[t * m + j] = kBinary ? exp(P.y[row] * wd) : exp(P.y[row] * wd * P.value[p]);
}

// a group per row: the row's list holds its sorted pairs in ascending index;
// those in [lo, hi) are the block's, and model j's live factors multiply into
// dual[row][j] in that order.  A (row, model) no live factor touches is not
// written.
__global__ __launch_bounds__(256) void dr_rows_kernel(
    const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ row_pair, uint32_t rows,
    uint32_t lo, uint32_t hi, uint32_t n, const double* __restrict__ factor, uint32_t m,
    uint32_t gs, double* __restrict__ dual) {
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t r = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  if (r >= rows || j >= m) return;
  const uint32_t e = row_start[r + 1] < n ? row_start[r + 1] : n;
  uint32_t a = row_start[r] < e ? row_start[r] : e;
  a += lower_bound(row_pair + a, e - a, lo);  // the first entry at or past lo
  double d = 0.0;
  bool touched = false;
  for (uint32_t l = a; l < e; ++l) {
    const uint32_t i = row_pair[l];
    if (i >= hi || i >= n) break;
    const double f = factor[(uint64_t)(i - lo) * m + j];
    if (f == -1.0) continue;
    if (!touched) d = dual[r * m + j];
    touched = true;
    d = d * f;
  }
  if (touched) dual[r * m + j] = d;
}

// ---- objv -------------------------------------------------------------------------
// log(1 + 1 / dual) per (row, model) (darling.cc:506); partial[workgroup][j] =
// darling_objv_kernel's tree over model j's 256 values.  The workgroup's
// 256 x m block is walked kObjvCols columns at a time, as logit_rows_kernel
// walks its block.
__global__ __launch_bounds__(256) void dr_objv_kernel(const double* __restrict__ dual,
                                                      uint32_t rows, uint32_t m,
                                                      double* __restrict__ partial) {
  __shared__ double s[kObjvCols][256];
  const uint32_t t = threadIdx.x;
  const uint64_t row0 = (uint64_t)blockIdx.x * 256u;
  for (uint32_t c0 = 0; c0 < m; c0 += kObjvCols) {
    const uint32_t w = m - c0 < (uint32_t)kObjvCols ? m - c0 : (uint32_t)kObjvCols;
    for (uint32_t el = t; el < 256u * w; el += 256u) {
      const uint32_t r = el / w, cc = el % w;
      const uint64_t i = row0 + r;
      s[cc][r] = i < rows ? log(1 + 1 / dual[i * m + c0 + cc]) : 0.0;
    }
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {  // dev::block_tree_sum's order, per column
      if ((int)t < h)
        for (uint32_t cc = 0; cc < w; ++cc) s[cc][t] += s[cc][t + h];
      __syncthreads();
    }
    if (t < w) partial[(uint64_t)blockIdx.x * m + c0 + t] = s[t][0];
    __syncthreads();
  }
}

// workgroup j: objv_kernel's order over model j's partials
__global__ __launch_bounds__(256) void dr_objv_final_kernel(const double* __restrict__ partial,
                                                            uint32_t nparts, uint32_t m,
                                                            double* __restrict__ objv) {
  __shared__ double s[256];
  double a = 0.0;
  for (uint32_t p = threadIdx.x; p < nparts; p += 256) a += partial[(uint64_t)p * m + blockIdx.x];
  dev::block_tree_sum(a, s);
  if (threadIdx.x == 0) objv[blockIdx.x] = s[0];
}

// ---- the server ---------------------------------------------------------------------
// Darling::updateWeight (darling.cc:437-477), a group per position, lane j
// model j: darling_kernel's operations on [n][m] arrays.  slots: kRowSlots
// rows of kDrMax words, zero on entry.
__global__ __launch_bounds__(256) void dr_server_kernel(
    const double* __restrict__ G, const double* __restrict__ U, double* __restrict__ w,
    double* __restrict__ delta, uint32_t* __restrict__ active, uint64_t n, uint32_t m,
    uint32_t gs, ServerParams P, unsigned long long* __restrict__ slots) {
  __shared__ unsigned long long vmax[256];
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  const bool in = i < n && j < m;
  const uint32_t word = i < n ? active[i] : 0u;
  bool bit = in && ((word >> j) & 1u);
  double vio = 0;
  if (bit) {
    const uint64_t at = i * m + j;
    const double lambda = P.lambda[j], kkt = P.kkt[j];
    const double g = G[at], u = U[at] / P.eta[j] + 1e-10;
    const double g_pos = g + lambda, g_neg = g - lambda;
    double wk = w[at];
    double d = -wk;
    bool inactive = false;
    if (wk == 0) {
      if (g_pos < 0) {
        vio = -g_pos;
      } else if (g_neg > 0) {
        vio = g_neg;
      } else if (g_pos > kkt && g_neg < -kkt) {
        inactive = true;
      }
    }
    if (inactive) {
      bit = false;
      w[at] = inactive_value();
    } else {
      if (g_pos <= u * wk) {
        d = -g_pos / u;
      } else if (g_neg >= u * wk) {
        d = -g_neg / u;
      }
      const double dk = delta[at];
      d = std_min(dk, std_max(-dk, d));
      delta[at] = std_min(P.delta_max[j], 2 * fabs(d) + .1);
      wk += d;
      w[at] = wk;
    }
  }
  // the new mask word: one ballot, one shift, one store; bits at or above m
  // stay as they were
  const uint32_t all = m == 32 ? 0xffffffffu : ((1u << m) - 1u);
  const uint32_t nw = (word & ~all) | group_ballot(bit, gs);
  if (j == 0 && i < n && nw != word) active[i] = nw;
  // the violation of model j: a max on bit patterns (every vio is a
  // non-negative double) over the workgroup's groups, which sit G apart
  vmax[threadIdx.x] = (unsigned long long)__double_as_longlong(vio);
  __syncthreads();
  for (uint32_t h = 128; h >= (1u << gs); h >>= 1) {
    if (threadIdx.x < h) {
      const unsigned long long o = vmax[threadIdx.x + h];
      if (o > vmax[threadIdx.x]) vmax[threadIdx.x] = o;
    }
    __syncthreads();
  }
  if (threadIdx.x < m && vmax[threadIdx.x])
    __hip_atomic_fetch_max(slots + (blockIdx.x % kRowSlots) * kDrMax + threadIdx.x,
                           vmax[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// workgroup j (one wave): the slot rows' max of model j folded into vio[j],
// violation_ = std::max(violation_, vio) (darling.cc:466); the slots back to zero
__global__ __launch_bounds__(kRowSlots) void dr_vio_kernel(unsigned long long* __restrict__ slots,
                                                           unsigned long long* __restrict__ vio) {
  const uint32_t at = threadIdx.x * kDrMax + blockIdx.x;
  unsigned long long vb = slots[at];
  slots[at] = 0;
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)vb, s, 64);
    vb = o > vb ? o : vb;
  }
  // the updates of one server run one after another: a plain read-modify-write
  if (threadIdx.x == 0 && vb > vio[blockIdx.x]) vio[blockIdx.x] = vb;
}

__global__ __launch_bounds__(256) void dr_zero_kernel(unsigned long long* __restrict__ p,
                                                      uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) p[i] = 0;
}

// evaluateProgress (darling.cc:538-555) per model, progress_kernel's order:
// psum[workgroup][j] = the tree sum of model j's 256 |w|, pcnt its count of
// live weights (w == w and w != 0), pact its count of set bits
__global__ __launch_bounds__(256) void dr_progress_kernel(
    const double* __restrict__ w, const uint32_t* __restrict__ active, uint64_t n, uint32_t m,
    double* __restrict__ psum, unsigned long long* __restrict__ pcnt,
    unsigned long long* __restrict__ pact) {
  __shared__ double s[256];
  __shared__ uint32_t wc[4], wa[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t word = i < n ? active[i] : 0u;
  for (uint32_t j = 0; j < m; ++j) {
    bool live = false;
    double a = 0.0;
    if (i < n) {
      const double x = w[i * m + j];
      live = x == x && x != 0;
      a = live ? fabs(x) : 0.0;
    }
    const unsigned long long bl = __ballot(live), ba = __ballot((word >> j) & 1u);
    if ((threadIdx.x & 63) == 0) {
      wc[threadIdx.x >> 6] = (uint32_t)__popcll(bl);
      wa[threadIdx.x >> 6] = (uint32_t)__popcll(ba);
    }
    dev::block_tree_sum(a, s);
    if (threadIdx.x == 0) {
      const uint64_t at = (uint64_t)blockIdx.x * m + j;
      psum[at] = s[0];
      pcnt[at] = (unsigned long long)wc[0] + wc[1] + wc[2] + wc[3];
      pact[at] = (unsigned long long)wa[0] + wa[1] + wa[2] + wa[3];
    }
    __syncthreads();
  }
}

// workgroup j: progress_final_kernel's order over model j's partials;
// res[3 j] = nnz_w, [3 j + 1] = the sum's bits, [3 j + 2] = the active count
__global__ __launch_bounds__(256) void dr_progress_final_kernel(
    const double* __restrict__ psum, const unsigned long long* __restrict__ pcnt,
    const unsigned long long* __restrict__ pact, uint64_t nparts, uint32_t m,
    unsigned long long* __restrict__ res) {
  __shared__ double s[256];
  __shared__ unsigned long long wc[4], wa[4];
  const uint32_t j = blockIdx.x;
  double a = 0.0;
  unsigned long long c = 0, ac = 0;
  for (uint64_t p = threadIdx.x; p < nparts; p += 256) {
    a += psum[p * m + j];
    c += pcnt[p * m + j];
    ac += pact[p * m + j];
  }
  for (int o = 32; o > 0; o >>= 1) {
    c += (unsigned long long)__shfl_xor((long long)c, o, 64);
    ac += (unsigned long long)__shfl_xor((long long)ac, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    wc[threadIdx.x >> 6] = c;
    wa[threadIdx.x >> 6] = ac;
  }
  dev::block_tree_sum(a, s);
  if (threadIdx.x == 0) {
    res[3 * j] = wc[0] + wc[1] + wc[2] + wc[3];
    res[3 * j + 1] = (unsigned long long)__double_as_longlong(s[0]);
    res[3 * j + 2] = wa[0] + wa[1] + wa[2] + wa[3];
  }
}

}  // namespace
}  // namespace psg

// ------------------------------------------------------------------- host --
using psg::fail;

namespace {

using namespace psg;

int drows_ready(psg_minibatch* mb, const char* who) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_LOCAL || mb->drows_m == 0)
    return fail(PSG_ERR_ARG, "%s before psg_mb_darling_rows_init", who);
  return PSG_OK;
}

int drows_block(psg_minibatch* mb, size_t cb, size_t ce, const char* who, uint32_t* lo,
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

Pairs pairs_of(const psg_minibatch* mb) {
  return Pairs{mb->spos, mb->at<uint32_t>(B_ROW_OF), mb->at<uint32_t>(B_RUN_OF),
               mb->at<uint32_t>(B_RUN_RANK), mb->binary ? nullptr : mb->at<double>(B_VALUE),
               mb->at<double>(B_Y), (uint32_t)mb->nnz, (uint32_t)mb->n_uniq, (uint32_t)mb->ndict,
               (uint32_t)mb->rows};
}

}  // namespace

namespace psg {

int darling_rows_read(psg_minibatch* mb, int what, void* out, size_t cap_bytes, size_t* n_out) {
  if (int rc = drows_ready(mb, "psg_mb_rows_read")) return rc;
  const size_t m = (size_t)mb->drows_m;
  int id;
  size_t n, first = 0, elem = 8;
  switch (what) {
    case PSG_MB_ROWS_DARLING_DUAL: id = B_DR_DUAL; n = mb->rows * m; break;
    case PSG_MB_ROWS_DARLING_CUR_W: id = B_DR_CUR_W; n = mb->ndict * m; break;
    case PSG_MB_ROWS_DARLING_DELTA: id = B_DR_DELTA; n = mb->ndict * m; break;
    case PSG_MB_ROWS_DARLING_DELTA_W:
      id = B_DR_DELTA_W; n = (mb->dr_last_ce - mb->dr_last_cb) * m; first = mb->dr_last_cb * m;
      break;
    case PSG_MB_ROWS_DARLING_MASK: id = B_DR_MASK; n = mb->ndict; elem = 4; break;
    default: return fail(PSG_ERR_ARG, "psg_mb_rows_read: array %d", what);
  }
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;
  *n_out = n;
  if (elem * n > cap_bytes)
    return fail(PSG_ERR_SIZE, "psg_mb_rows_read: array %d holds %zu bytes, room for %zu", what,
                elem * n, cap_bytes);
  if (n == 0) return PSG_OK;
  if (!out) return fail(PSG_ERR_ARG, "null output");
  HIP_TRY(hipMemcpy(out, (const char*)mb->b[id].p + first * elem, elem * n,
                    hipMemcpyDeviceToHost));
  return PSG_OK;
}

}  // namespace psg

extern "C" {

int psg_mb_darling_rows_init(psg_minibatch* mb, int m, double delta_init, const double* w_dev,
                             void* stream) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (m < 1 || m > kDrMax)
    return fail(PSG_ERR_ARG, "psg_mb_darling_rows_init: %d models: 1 .. %d", m, kDrMax);
  if (mb->state < S_LOCAL)
    return fail(PSG_ERR_ARG, "psg_mb_darling_rows_init before psg_mb_localize");
  HIP_TRY(hipSetDevice(mb->device));
  mb->drows_m = 0;
  const size_t rows_z = mb->rows, n_z = mb->nnz, nd_z = mb->ndict, mz = (size_t)m;
  const uint32_t nparts = blocks_of(rows_z, 256);
  if (int rc = mb->need_all({
      {B_DR_DUAL, 8 * rows_z * mz}, {B_DR_CUR_W, 8 * nd_z * mz}, {B_DR_DELTA, 8 * nd_z * mz},
      {B_DR_DELTA_W, 8 * nd_z * mz}, {B_DR_EXPD, mb->binary ? 8 * nd_z * mz : 0},
      {B_DR_MASK, 4 * nd_z}, {B_DR_YTAU, 8 * rows_z * mz}, {B_DR_Q, 8 * rows_z * mz},
      {B_DR_PARTIAL, 8 * (size_t)nparts * mz + 8}, {B_DR_OBJV, 8 * mz},
      {B_RKEY_A, 8 * n_z}, {B_RKEY_B, 8 * n_z}, {B_RPOS_A, 4 * n_z}, {B_RPOS_B, 4 * n_z},
      {B_ROW_START, 4 * (rows_z + 1)}, {B_COL_RANGE, 8 * nd_z}}))
    return rc;
  hipStream_t s = mb->pick(stream);
  // dual = exp(y .* (Z w)) per model, darling.cc:110: Z w by the rows product
  if (rows_z && w_dev)
    if (int rc = psg_mb_times_rows(mb, w_dev, m, mb->at<double>(B_DR_DUAL), s)) return rc;
  if (int rc = mb->order(s)) return rc;
  const uint32_t n = (uint32_t)n_z, nd = (uint32_t)nd_z, nu = (uint32_t)mb->n_uniq;
  const uint32_t rows = (uint32_t)rows_z;
  if (rows) {
    if (w_dev)
      LAUNCH(dr_dual_init_kernel, blocks_of(rows_z * mz, 256), s, mb->at<double>(B_Y), rows,
             (uint32_t)m, mb->at<double>(B_DR_DUAL));
    else
      LAUNCH(dr_fill_kernel, blocks_of(rows_z * mz, 256), s, mb->at<double>(B_DR_DUAL),
             (uint64_t)(rows_z * mz), 1.0);
  }
  if (nd) {
    const uint64_t ne = nd_z * mz;
    if (w_dev)
      LAUNCH(dr_copy_kernel, blocks_of(ne, 256), s, mb->at<double>(B_DR_CUR_W), w_dev, ne);
    else
      LAUNCH(dr_fill_kernel, blocks_of(ne, 256), s, mb->at<double>(B_DR_CUR_W), ne, 0.0);
    LAUNCH(dr_fill_kernel, blocks_of(ne, 256), s, mb->at<double>(B_DR_DELTA_W), ne, 0.0);
    LAUNCH(dr_fill_kernel, blocks_of(ne, 256), s, mb->at<double>(B_DR_DELTA), ne, delta_init);
    LAUNCH(dr_mask_fill_kernel, blocks_of(nd, 256), s, mb->at<uint32_t>(B_DR_MASK), nd,
           m == 32 ? 0xffffffffu : ((1u << m) - 1u));  // :114
    LAUNCH(dr_col_range_kernel, blocks_of(nd, 256), s, mb->at<uint32_t>(B_DICT_RUN), nd,
           mb->at<uint32_t>(B_RUN_START), nu, n, mb->at<uint32_t>(B_COL_RANGE));
  }
  // the rows' lists: the sorted pairs, stably sorted by row.  The scalar
  // state's lists are these, in these blocks: a rebuild writes the same words.
  const uint32_t* row_pair = nullptr;
  if (n) {
    uint64_t* rkey = mb->at<uint64_t>(B_RKEY_B);
    LAUNCH(dr_row_key_kernel, blocks_of(n, 256), s, pairs_of(mb), rkey);
    uint64_t differ = 1;
    while (differ <= rows) differ <<= 1;
    const SortBuffers b{mb->at<uint64_t>(B_RKEY_A), mb->at<uint64_t>(B_RKEY_B),
                        mb->at<uint32_t>(B_RPOS_A), mb->at<uint32_t>(B_RPOS_B),
                        mb->at<uint32_t>(B_COUNTS), mb->d_dtotal()};
    const uint64_t* sorted_row = nullptr;
    if (int rc = enqueue_radix_sort(rkey, n, differ - 1, b, &sorted_row, &row_pair, s)) return rc;
    LAUNCH(dr_row_start_kernel, blocks_of((uint64_t)rows + 1, 256), s, sorted_row, n, rows,
           mb->at<uint32_t>(B_ROW_START));
  } else {
    LAUNCH(dr_mask_fill_kernel, blocks_of(rows_z + 1, 256), s, mb->at<uint32_t>(B_ROW_START),
           rows + 1, 0u);
  }
  if (int rc = launched("darling rows init")) return rc;
  if (int rc = mb->mark(s)) return rc;
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
  if (mb->h_small[2]) {  // as psg_mb_gradient: localize again
    mb->state = S_UNIQ;
    return fail(PSG_ERR_UNSORTED, "%llu key pairs of the dictionary not strictly increasing",
                mb->h_small[2]);
  }
  mb->pair_lo[nd_z] = n;
  for (size_t k = nd_z; k-- > 0;)
    mb->pair_lo[k] = range[2 * k] < range[2 * k + 1] ? range[2 * k] : mb->pair_lo[k + 1];
  mb->pair_hi[0] = 0;
  for (size_t k = 0; k < nd_z; ++k)
    mb->pair_hi[k + 1] = range[2 * k] < range[2 * k + 1] ? range[2 * k + 1] : mb->pair_hi[k];
  mb->n_long = std::min<size_t>((uint32_t)(mb->h_small[5] & 0xffffffffu), nd_z);
  mb->row_pair = row_pair;
  mb->dr_last_cb = mb->dr_last_ce = 0;
  mb->drows_m = m;
  return PSG_OK;
}

int psg_mb_darling_rows_reset_active(psg_minibatch* mb, void* stream) {
  if (int rc = drows_ready(mb, "psg_mb_darling_rows_reset_active")) return rc;
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  const int m = mb->drows_m;
  if (mb->ndict)
    LAUNCH(dr_mask_fill_kernel, blocks_of(mb->ndict, 256), s, mb->at<uint32_t>(B_DR_MASK),
           (uint32_t)mb->ndict, m == 32 ? 0xffffffffu : ((1u << m) - 1u));
  if (int rc = launched("darling rows reset_active")) return rc;
  return mb->mark(s);
}

int psg_mb_darling_rows_gradients(psg_minibatch* mb, size_t cb, size_t ce, double* g_dev,
                                  double* u_dev, void* stream) {
  if (int rc = drows_ready(mb, "psg_mb_darling_rows_gradients")) return rc;
  uint32_t lo, hi;
  if (int rc = drows_block(mb, cb, ce, "psg_mb_darling_rows_gradients", &lo, &hi)) return rc;
  if (cb < ce && (!g_dev || !u_dev)) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  const uint32_t m = (uint32_t)mb->drows_m, gs = group_shift((int)m), per = 256u >> gs;
  if (int rc = mb->need(B_DR_TERM, 16 * (size_t)(hi - lo) * m)) return rc;
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  if (cb == ce) return mb->mark(s);
  const uint32_t n = (uint32_t)mb->nnz, nd = (uint32_t)mb->ndict, nu = (uint32_t)mb->n_uniq;
  const uint32_t b = (uint32_t)cb, e = (uint32_t)ce, rows = (uint32_t)mb->rows;
  const uint32_t* mask = mb->at<uint32_t>(B_DR_MASK);
  double2* term = mb->at<double2>(B_DR_TERM);
  if (mb->binary)
    LAUNCH(dr_exp_delta_kernel, blocks_of((uint64_t)(e - b) * m, 256), s,
           mb->at<double>(B_DR_DELTA), mask, b, e, m, mb->at<double>(B_DR_EXPD));
  if (hi > lo) {
    LAUNCH(dr_table_kernel, blocks_of((uint64_t)rows * m, 256), s, mb->at<double>(B_Y),
           mb->at<double>(B_DR_DUAL), rows, m, mb->at<double>(B_DR_YTAU), mb->at<double>(B_DR_Q));
    if (mb->binary)
      LAUNCH(dr_terms_kernel<true>, blocks_of(hi - lo, per), s, pairs_of(mb), mask,
             mb->at<double>(B_DR_YTAU), mb->at<double>(B_DR_Q), mb->at<double>(B_DR_EXPD), lo, hi,
             m, gs, term);
    else
      LAUNCH(dr_terms_kernel<false>, blocks_of(hi - lo, per), s, pairs_of(mb), mask,
             mb->at<double>(B_DR_YTAU), mb->at<double>(B_DR_Q), mb->at<double>(B_DR_DELTA), lo, hi,
             m, gs, term);
  }
  LAUNCH(dr_sum_short_kernel, blocks_of(e - b, per), s, mb->at<uint32_t>(B_DICT_RUN), nd,
         mb->at<uint32_t>(B_RUN_START), nu, n, mask, b, e, lo, hi, term, m, gs, g_dev, u_dev);
  if (hi - lo > kLongRun && mb->n_long)
    LAUNCH(dr_sum_long_kernel, std::min<uint32_t>(blocks_of(mb->n_long, 4), kLongGrid), s,
           mb->at<uint32_t>(B_LONG_LIST), (const uint32_t*)(mb->d_small + 5),
           mb->at<uint32_t>(B_DICT_RUN), nd, mb->at<uint32_t>(B_RUN_START), nu, n, mask, b, e, lo,
           hi, term, m, g_dev, u_dev);
  if (int rc = launched("darling rows gradients")) return rc;
  return mb->mark(s);
}

int psg_mb_darling_rows_update_dual(psg_minibatch* mb, size_t cb, size_t ce,
                                    const double* new_w_dev, const double* delta_max,
                                    void* stream) {
  if (int rc = drows_ready(mb, "psg_mb_darling_rows_update_dual")) return rc;
  uint32_t lo, hi;
  if (int rc = drows_block(mb, cb, ce, "psg_mb_darling_rows_update_dual", &lo, &hi)) return rc;
  if (!delta_max || (cb < ce && !new_w_dev)) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  const uint32_t m = (uint32_t)mb->drows_m, gs = group_shift((int)m), per = 256u >> gs;
  if (int rc = mb->need(B_DR_TERM, 16 * (size_t)(hi - lo) * m)) return rc;
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  mb->dr_last_cb = cb;
  mb->dr_last_ce = ce;
  if (cb == ce) return mb->mark(s);
  const uint32_t n = (uint32_t)mb->nnz, rows = (uint32_t)mb->rows;
  uint32_t* mask = mb->at<uint32_t>(B_DR_MASK);
  double* factor = mb->at<double>(B_DR_TERM);
  PerModel dm;
  for (uint32_t j = 0; j < (uint32_t)kDrMax; ++j) dm.v[j] = j < m ? delta_max[j] : 0.0;
  LAUNCH(dr_state_kernel, blocks_of(ce - cb, per), s, new_w_dev, (uint32_t)cb, (uint32_t)ce, m, gs,
         dm, mb->at<double>(B_DR_CUR_W), mb->at<double>(B_DR_DELTA), mask,
         mb->at<double>(B_DR_DELTA_W));
  if (hi > lo && rows) {
    if (mb->binary)
      LAUNCH(dr_factor_kernel<true>, blocks_of(hi - lo, per), s, pairs_of(mb), mask,
             mb->at<double>(B_DR_DELTA_W), lo, hi, m, gs, factor);
    else
      LAUNCH(dr_factor_kernel<false>, blocks_of(hi - lo, per), s, pairs_of(mb), mask,
             mb->at<double>(B_DR_DELTA_W), lo, hi, m, gs, factor);
    LAUNCH(dr_rows_kernel, blocks_of(rows, per), s, mb->at<uint32_t>(B_ROW_START), mb->row_pair,
           rows, lo, hi, n, factor, m, gs, mb->at<double>(B_DR_DUAL));
  }
  if (int rc = launched("darling rows update_dual")) return rc;
  return mb->mark(s);
}

int psg_mb_darling_rows_objv(psg_minibatch* mb, double* objv, void* stream) {
  if (int rc = drows_ready(mb, "psg_mb_darling_rows_objv")) return rc;
  if (!objv) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  const uint32_t m = (uint32_t)mb->drows_m;
  const uint32_t rows = (uint32_t)mb->rows, nparts = blocks_of(rows, 256);
  if (rows)
    LAUNCH(dr_objv_kernel, nparts, s, mb->at<double>(B_DR_DUAL), rows, m,
           mb->at<double>(B_DR_PARTIAL));
  LAUNCH(dr_objv_final_kernel, m, s, mb->at<double>(B_DR_PARTIAL), nparts, m,
         mb->at<double>(B_DR_OBJV));
  if (int rc = launched("darling rows objv")) return rc;
  if (int rc = mb->mark(s)) return rc;
  double h[kDrMax];
  HIP_TRY(hipMemcpyAsync(h, mb->b[B_DR_OBJV].p, 8 * (size_t)m, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  memcpy(objv, h, 8 * (size_t)m);
  return PSG_OK;
}

int psg_mb_darling_rows_set_state(psg_minibatch* mb, int m, const double* dual,
                                  const double* cur_w, const double* delta,
                                  const uint32_t* mask) {
  if (int rc = drows_ready(mb, "psg_mb_darling_rows_set_state")) return rc;
  if (m != mb->drows_m)
    return fail(PSG_ERR_ARG, "psg_mb_darling_rows_set_state: arrays of %d models, a state of %d",
                m, mb->drows_m);
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;
  const size_t mz = (size_t)m;
  if (mask && mb->ndict && m < 32)
    for (size_t k = 0; k < mb->ndict; ++k)
      if (mask[k] >> m)
        return fail(PSG_ERR_ARG, "mask[%zu] = %#x has a bit at or above %d", k, mask[k], m);
  if (dual && mb->rows)
    HIP_TRY(hipMemcpy(mb->b[B_DR_DUAL].p, dual, 8 * mb->rows * mz, hipMemcpyHostToDevice));
  if (cur_w && mb->ndict)
    HIP_TRY(hipMemcpy(mb->b[B_DR_CUR_W].p, cur_w, 8 * mb->ndict * mz, hipMemcpyHostToDevice));
  if (delta && mb->ndict)
    HIP_TRY(hipMemcpy(mb->b[B_DR_DELTA].p, delta, 8 * mb->ndict * mz, hipMemcpyHostToDevice));
  if (mask && mb->ndict)
    HIP_TRY(hipMemcpy(mb->b[B_DR_MASK].p, mask, 4 * mb->ndict, hipMemcpyHostToDevice));
  return PSG_OK;
}

// ---- the server -----------------------------------------------------------------
int psg_darling_rows_update_dev(psg_ctx* c, const double* G_dev, const double* U_dev,
                                double* w_dev, double* delta_dev, uint32_t* active_dev, size_t n,
                                int m, const psg_darling_param* params, double* vio_dev,
                                void* stream) {
  if (!c || !params || !vio_dev) return fail(PSG_ERR_ARG, "null argument");
  if (m < 1 || m > kDrMax)
    return fail(PSG_ERR_ARG, "psg_darling_rows_update_dev: %d models: 1 .. %d", m, kDrMax);
  if (n && (!G_dev || !U_dev || !w_dev || !delta_dev || !active_dev))
    return fail(PSG_ERR_ARG, "null argument");
  if (n >= (1ull << 32)) return fail(PSG_ERR_SIZE, "%zu positions >= 2^32", n);
  std::lock_guard<std::mutex> l(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (!c->d_vio_rows) {  // the slot rows, zero between updates
    HIP_TRY(hipMalloc((void**)&c->d_vio_rows, 8 * kRowSlots * kDrMax));
    LAUNCH(dr_zero_kernel, blocks_of(kRowSlots * kDrMax, 256), s, c->d_vio_rows,
           (uint32_t)(kRowSlots * kDrMax));
  }
  ServerParams P;
  for (int j = 0; j < kDrMax; ++j) {
    const psg_darling_param& p = params[j < m ? j : 0];
    P.eta[j] = p.eta;
    P.lambda[j] = p.lambda;
    P.kkt[j] = p.kkt_filter_threshold;
    P.delta_max[j] = p.delta_max;
  }
  const uint32_t gs = group_shift(m);
  if (n) {
    LAUNCH(dr_server_kernel, blocks_of(n, 256u >> gs), s, G_dev, U_dev, w_dev, delta_dev,
           active_dev, (uint64_t)n, (uint32_t)m, gs, P, c->d_vio_rows);
    hipLaunchKernelGGL(dr_vio_kernel, dim3(m), dim3(kRowSlots), 0, s, c->d_vio_rows,
                       (unsigned long long*)vio_dev);
  }
  return launched("darling rows update");
}

int psg_darling_rows_progress(psg_ctx* c, const double* w_dev, const uint32_t* active_dev,
                              size_t n, int m, size_t* nnz_w, double* sum_abs, size_t* nnz_active,
                              void* stream) {
  if (!c) return fail(PSG_ERR_ARG, "null argument");
  if (m < 1 || m > kDrMax)
    return fail(PSG_ERR_ARG, "psg_darling_rows_progress: %d models: 1 .. %d", m, kDrMax);
  if (n && (!w_dev || !active_dev)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const size_t nparts = (n + 255) / 256, mz = (size_t)m;
  // once per pass, and it waits anyway: a block of its own for the partials
  unsigned long long* work = nullptr;
  HIP_TRY(hipMalloc((void**)&work, 8 * (3 * nparts * mz + 3 * mz) + 8));
  unsigned long long* res = work + 3 * nparts * mz;
  if (n)
    LAUNCH(dr_progress_kernel, (uint32_t)nparts, s, w_dev, active_dev, (uint64_t)n, (uint32_t)m,
           (double*)work, work + nparts * mz, work + 2 * nparts * mz);
  LAUNCH(dr_progress_final_kernel, m, s, (const double*)work, work + nparts * mz,
         work + 2 * nparts * mz, (uint64_t)nparts, (uint32_t)m, res);
  unsigned long long h[3 * kDrMax];
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h, res, 24 * mz, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(work);
  if (e != hipSuccess) return fail(PSG_ERR_DEVICE, "darling rows progress: %s", hipGetErrorString(e));
  for (int j = 0; j < m; ++j) {
    if (nnz_w) nnz_w[j] = (size_t)h[3 * j];
    if (sum_abs) memcpy(sum_abs + j, h + 3 * j + 1, 8);
    if (nnz_active) nnz_active[j] = (size_t)h[3 * j + 2];
  }
  return PSG_OK;
}

}  // extern "C"
