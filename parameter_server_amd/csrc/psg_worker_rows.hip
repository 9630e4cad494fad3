// psg_worker_rows.hip -- the products and the loss of psg_worker.hip for m
// models at once (psg_mb_times_rows, psg_mb_trans_times_rows,
// psg_mb_gradient_rows; include/psg.h): the pulled weights are a row of m
// values per dictionary key, Xw, tau and c a row per example, the gradient a
// row per key, all row-major.  The sort, the localizer and countKeys do not
// depend on the model and are psg_worker.hip's, run once.
//
// Column j of every output is bit for bit the scalar kernels' result for
// column j alone: one rounded multiply and one rounded add per entry, the
// terms in the same order on one accumulator per column, and objv[j] by the
// same tree over each 256 rows and the same second reduction.
//
// Work split: a group of G lanes (the power of two >= m) owns one row of Z
// (times) or one dictionary key (trans_times); lane j of the group keeps
// column j's accumulator.  The index, value and position words are the same
// address in every lane of a group (one broadcast read), the x or c row is
// one contiguous read of 8 m bytes.  times issues kRowsAhead entries' loads
// ahead of the add chain; their addresses do not depend on the accumulator.
// trans_times writes the n x m term rows first, as the scalar path writes its
// n terms: gathering the c row of row_of[spos[i]] inside the ordered sum was
// measured and lost ten to one on the head key's run, whose
// one wave then waits on three dependent gathers per step.  A run longer than
// kLongRun (psg_worker.hip's list, built at localize) goes to a whole wave,
// which streams the run's contiguous term rows through LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include "../../include/psg.h"
#include "psg_blocks.h"
#include "psg_colsum.h"
#include "psg_device.h"
#include "psg_ftrl_rows.h"
#include "psg_host.h"
#include "psg_internal.h"
#include "psg_minibatch.h"
#include "psg_sort.h"

namespace psg {
namespace {

#ifndef PSG_ROWS_AHEAD
#define PSG_ROWS_AHEAD 4  // entries of a row of Z loaded ahead of the adds
#endif
constexpr int kRowsAhead = PSG_ROWS_AHEAD;
#ifndef PSG_ROWS_LONG_AHEAD
#define PSG_ROWS_LONG_AHEAD 8  // loads of 64 doubles a long run's wave keeps ahead of its adds
#endif
constexpr int kLongAhead = PSG_ROWS_LONG_AHEAD;
constexpr int kLossCols = 8;  // columns per pass of the loss kernel's LDS block

// the run [*b, *e) of sorted pairs of dictionary key k, and the row of a
// sorted pair, clamped as in psg_worker.hip (which keeps its own copies: its
// kernels are not touched)
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

struct Pairs {  // the sorted pairs of the minibatch and what they point at
  const uint32_t* spos;
  const uint32_t* row_of;
  const double* value;  // null: binary
  uint32_t n, rows;
};

// c[row of pair i][j] (* value of pair i): the term of column j
__device__ __forceinline__ double pair_term(const Pairs& P, const double* __restrict__ c,
                                            uint32_t m, uint32_t j, uint64_t i) {
  uint32_t p = P.spos[i];
  if (p >= P.n) p = 0;
  uint32_t row = P.row_of[p];
  if (row >= P.rows) row = 0;
  const double cv = c[(uint64_t)row * m + j];
  return P.value ? cv * P.value[p] : cv;
}

// times, row-major (sparse_matrix.h:75-86): a group per row of Z
__global__ __launch_bounds__(256) void times_rows_kernel(
    const uint64_t* __restrict__ new_offset, const uint32_t* __restrict__ new_index,
    const double* __restrict__ new_value, uint32_t rows, uint32_t ndict,
    const double* __restrict__ x, uint32_t m, uint32_t gs, double* __restrict__ xw) {
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t r = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  if (r >= rows || j >= m) return;
  const uint64_t b = new_offset[r], e = new_offset[r + 1];
  double acc = 0.0;
  uint64_t i = b;
  for (; i + kRowsAhead <= e; i += kRowsAhead) {
    double xv[kRowsAhead], v[kRowsAhead];
#pragma unroll
    for (int u = 0; u < kRowsAhead; ++u) {
      uint32_t k = new_index[i + u];
      if (k >= ndict) k = 0;  // never: ranks of the dictionary
      xv[u] = x[(uint64_t)k * m + j];
      v[u] = new_value ? new_value[i + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kRowsAhead; ++u) acc = new_value ? acc + xv[u] * v[u] : acc + xv[u];
  }
  for (; i < e; ++i) {
    uint32_t k = new_index[i];
    if (k >= ndict) k = 0;
    const double xv = x[(uint64_t)k * m + j];
    acc = new_value ? acc + xv * new_value[i] : acc + xv;
  }
  xw[r * m + j] = acc;  // an empty row: +0.0
}

// transTimes in three launches, as psg_worker.hip's: the term row of every
// sorted pair first (a group per pair: all the gathers, fully parallel, the
// rows written side by side in run order), then the ordered sums, which
// stream the term rows: a group per dictionary key for the runs up to
// kLongRun (and the keys with no run: +0.0) ...
__global__ __launch_bounds__(256) void terms_rows_kernel(Pairs P, const double* __restrict__ c,
                                                         uint32_t m, uint32_t gs,
                                                         double* __restrict__ term) {
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  if (i >= P.n || j >= m) return;
  term[i * m + j] = pair_term(P, c, m, j, i);
}

__global__ __launch_bounds__(256) void trans_rows_short_kernel(
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, const double* __restrict__ term, uint32_t m, uint32_t gs,
    double* __restrict__ g) {
  const uint32_t j = threadIdx.x & ((1u << gs) - 1);
  const uint64_t k = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> gs;
  if (k >= ndict || j >= m) return;
  uint32_t b, e;
  run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
  if (e - b > kLongRun) return;  // trans_rows_long_kernel's
  double acc = 0.0;
  for (uint64_t i = b; i < e; ++i) acc = acc + term[i * m + j];
  g[k * m + j] = acc;
}

// ... and a whole wave for a longer run: wave w of the launch takes
// long_list[w], [w + waves], ...  The run's term rows are one contiguous piece
// of memory; the wave copies it 64 doubles per load, kLongAhead loads ahead,
// into its LDS block, whole pairs at a time ([pair][m]), and lanes j < m add
// their column from there, one term after the other.
__global__ __launch_bounds__(256) void trans_rows_long_kernel(
    const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ count,
    const uint32_t* __restrict__ dict_run, uint32_t ndict, const uint32_t* __restrict__ run_start,
    uint32_t n_uniq, uint32_t n, const double* __restrict__ term, uint32_t m,
    double* __restrict__ g) {
  __shared__ double stage[4][64 * kLongAhead];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t pps = (64u * kLongAhead) / m, span = pps * m;  // pairs, doubles per refill
  const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), waves = gridDim.x * 4u;
  double* st = stage[threadIdx.x >> 6];
  const uint32_t nl = *count < ndict ? *count : ndict;
  for (uint32_t jl = wave; jl < nl; jl += waves) {
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)long_list[jl]);
    if (k >= ndict) continue;
    uint32_t b, e;
    run_of_key(k, ndict, dict_run, run_start, n_uniq, n, &b, &e);
    const uint64_t tb = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)b) * m;
    const uint64_t te = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)e) * m;
    double a = 0.0, cur[kLongAhead], nxt[kLongAhead];
#pragma unroll
    for (int u = 0; u < kLongAhead; ++u) {
      const uint32_t off = (uint32_t)u * 64u + lane;
      cur[u] = off < span && tb + off < te ? term[tb + off] : 0.0;
      nxt[u] = 0.0;
    }
    for (uint64_t base = tb; base < te; base += span) {
      const uint64_t ahead = base + span;
      if (ahead < te) {
#pragma unroll
        for (int u = 0; u < kLongAhead; ++u) {
          const uint32_t off = (uint32_t)u * 64u + lane;
          nxt[u] = off < span && ahead + off < te ? term[ahead + off] : 0.0;
        }
      }
      // LDS operations of one wave run in order; the fences keep the compiler
      // from moving the reads across the writes (as chain_sum, psg_worker.hip)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int u = 0; u < kLongAhead; ++u) st[u * 64 + lane] = cur[u];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint64_t left = (te - base) / m;
      const uint32_t cnt = left < pps ? (uint32_t)left : pps;
      if (lane < m) {  // eight LDS reads in flight ahead of the adds
        const double* col = st + lane;
        uint32_t t = 0;
        for (; t + 8 <= cnt; t += 8, col += 8 * m) {
          double v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = col[u * m];
#pragma unroll
          for (int u = 0; u < 8; ++u) a = a + v[u];
        }
        for (; t < cnt; ++t, col += m) a = a + *col;
      }
#pragma unroll
      for (int u = 0; u < kLongAhead; ++u) cur[u] = nxt[u];
    }
    if (lane < m) g[(uint64_t)k * m + lane] = a;
  }
}

// loss.h:74,81 per (row, model), as logit_kernel writes them; partial
// [workgroup][j] = the tree sum of model j's 256 losses.  The workgroup's
// 256 x m block is walked kLossCols columns at a time: element e of a pass is
// row e / w, column e % w (w columns in the pass), so a row's part is one
// contiguous piece; its losses go to LDS as [column][row] for the trees.
__global__ __launch_bounds__(256) void logit_rows_kernel(
    const double* __restrict__ y, const double* __restrict__ xw, uint32_t rows, uint32_t m,
    double* __restrict__ tau, double* __restrict__ c, double* __restrict__ loss,
    double* __restrict__ partial) {
  __shared__ double s[kLossCols][256];
  const uint32_t t = threadIdx.x;
  const uint64_t row0 = (uint64_t)blockIdx.x * 256u;
  for (uint32_t c0 = 0; c0 < m; c0 += kLossCols) {
    const uint32_t w = m - c0 < (uint32_t)kLossCols ? m - c0 : (uint32_t)kLossCols;
    for (uint32_t el = t; el < 256u * w; el += 256u) {
      const uint32_t r = el / w, cc = el % w;
      const uint64_t i = row0 + r;
      double l = 0.0;
      if (i < rows) {
        const uint64_t at = i * m + c0 + cc;
        const double yi = y[i], x = xw[at];
        const double tt = 1 / (1 + exp(yi * x));
        l = log(1 + exp(-yi * x));
        tau[at] = tt;
        c[at] = -yi * tt;
        loss[at] = l;
      }
      s[cc][r] = l;
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
__global__ __launch_bounds__(256) void objv_rows_kernel(const double* __restrict__ partial,
                                                        uint32_t nparts, uint32_t m,
                                                        double* __restrict__ objv) {
  __shared__ double s[256];
  double a = 0.0;
  for (uint32_t p = threadIdx.x; p < nparts; p += 256) a += partial[(uint64_t)p * m + blockIdx.x];
  dev::block_tree_sum(a, s);
  if (threadIdx.x == 0) objv[blockIdx.x] = s[0];
}

}  // namespace
}  // namespace psg

// ------------------------------------------------------------------- host --
using psg::fail;

namespace {

using namespace psg;

int rows_ready(psg_minibatch* mb, int m, const char* who) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (m < 1 || m > PSG_FTRL_MAX_MODELS)
    return fail(PSG_ERR_ARG, "%s: %d models: 1 .. %d", who, m, PSG_FTRL_MAX_MODELS);
  if (mb->state < S_LOCAL) return fail(PSG_ERR_ARG, "%s before psg_mb_localize", who);
  return PSG_OK;
}

int enqueue_times_rows(psg_minibatch* mb, const double* x, int m, double* xw, hipStream_t s) {
  const uint32_t gs = group_shift(m);
  if (mb->rows)
    LAUNCH(times_rows_kernel, blocks_of(mb->rows, 256u >> gs), s, mb->at<uint64_t>(B_NEW_OFFSET),
           mb->at<uint32_t>(B_NEW_INDEX), mb->binary ? nullptr : mb->at<double>(B_NEW_VALUE),
           (uint32_t)mb->rows, (uint32_t)mb->ndict, x, (uint32_t)m, gs, xw);
  return launched("times_rows");
}

int enqueue_trans_times_rows(psg_minibatch* mb, const double* c, int m, double* g, hipStream_t s) {
  const uint32_t n = (uint32_t)mb->nnz, nd = (uint32_t)mb->ndict, nu = (uint32_t)mb->n_uniq;
  const uint32_t gs = group_shift(m);
  if (nd) {
    const Pairs P{mb->spos, mb->at<uint32_t>(B_ROW_OF),
                  mb->binary ? nullptr : mb->at<double>(B_VALUE), n, (uint32_t)mb->rows};
    double* term = mb->at<double>(B_R_TERM);
    if (n) LAUNCH(terms_rows_kernel, blocks_of(n, 256u >> gs), s, P, c, (uint32_t)m, gs, term);
    LAUNCH(trans_rows_short_kernel, blocks_of(nd, 256u >> gs), s, mb->at<uint32_t>(B_DICT_RUN), nd,
           mb->at<uint32_t>(B_RUN_START), nu, n, term, (uint32_t)m, gs, g);
    if (n && mb->sum_order == PSG_SUM_BLOCKED) {
      if (int rc = colsum_enqueue(mb, term, m, g, nullptr, 0, nd, nullptr, nd, s)) return rc;
    } else if (n)
      LAUNCH(trans_rows_long_kernel, std::min<uint32_t>(blocks_of(nd, 4), kLongGrid), s,
             mb->at<uint32_t>(B_LONG_LIST), (const uint32_t*)(mb->d_small + 5),
             mb->at<uint32_t>(B_DICT_RUN), nd, mb->at<uint32_t>(B_RUN_START), nu, n, term,
             (uint32_t)m, g);
  }
  return launched("trans_times_rows");
}

}  // namespace

extern "C" {

int psg_mb_times_rows(psg_minibatch* mb, const double* x_dev, int m, double* xw_dev,
                      void* stream) {
  if (int rc = rows_ready(mb, m, "psg_mb_times_rows")) return rc;
  if ((mb->ndict && !x_dev) || (mb->rows && !xw_dev)) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  if (int rc = enqueue_times_rows(mb, x_dev, m, xw_dev, s)) return rc;
  return mb->mark(s);
}

int psg_mb_trans_times_rows(psg_minibatch* mb, const double* c_dev, int m, double* g_dev,
                            void* stream) {
  if (int rc = rows_ready(mb, m, "psg_mb_trans_times_rows")) return rc;
  if ((mb->rows && !c_dev) || (mb->ndict && !g_dev)) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->need(B_R_TERM, 8 * mb->nnz * (size_t)m)) return rc;
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  if (int rc = enqueue_trans_times_rows(mb, c_dev, m, g_dev, s)) return rc;
  return mb->mark(s);
}

int psg_mb_gradient_rows(psg_minibatch* mb, int loss, const double* w_dev, int m,
                         const double** grad_dev, double* objv, void* stream) {
  if (int rc = rows_ready(mb, m, "psg_mb_gradient_rows")) return rc;
  if (loss != PSG_LOSS_LOGIT) return fail(PSG_ERR_ARG, "loss %d: only PSG_LOSS_LOGIT is built", loss);
  if (mb->ndict && !w_dev) return fail(PSG_ERR_ARG, "null weights");
  HIP_TRY(hipSetDevice(mb->device));
  const uint32_t rows = (uint32_t)mb->rows, nparts = blocks_of(rows, 256);
  const size_t rm = 8 * mb->rows * (size_t)m;
  mb->rows_m = 0;
  if (int rc = mb->need_all({{B_R_XW, rm}, {B_R_TAU, rm}, {B_R_C, rm}, {B_R_LOSS, rm},
                             {B_R_PARTIAL, 8 * (size_t)nparts * m + 8},
                             {B_R_GRAD, 8 * mb->ndict * (size_t)m}, {B_R_OBJV, 8 * (size_t)m},
                             {B_R_TERM, 8 * mb->nnz * (size_t)m}}))
    return rc;
  hipStream_t s = mb->pick(stream);
  if (int rc = mb->order(s)) return rc;
  mb->tick(PSG_MB_STAGE_TIMES, 0, s);
  if (int rc = enqueue_times_rows(mb, w_dev, m, mb->at<double>(B_R_XW), s)) return rc;
  mb->tick(PSG_MB_STAGE_TIMES, 1, s);
  mb->tick(PSG_MB_STAGE_LOGIT, 0, s);
  if (rows)
    LAUNCH(logit_rows_kernel, nparts, s, mb->at<double>(B_Y), mb->at<double>(B_R_XW), rows,
           (uint32_t)m, mb->at<double>(B_R_TAU), mb->at<double>(B_R_C), mb->at<double>(B_R_LOSS),
           mb->at<double>(B_R_PARTIAL));
  LAUNCH(objv_rows_kernel, m, s, mb->at<double>(B_R_PARTIAL), nparts, (uint32_t)m,
         mb->at<double>(B_R_OBJV));
  mb->tick(PSG_MB_STAGE_LOGIT, 1, s);
  if (int rc = launched("logit_rows")) return rc;
  mb->tick(PSG_MB_STAGE_TRANS_TIMES, 0, s);
  if (int rc = enqueue_trans_times_rows(mb, mb->at<double>(B_R_C), m, mb->at<double>(B_R_GRAD), s))
    return rc;
  mb->tick(PSG_MB_STAGE_TRANS_TIMES, 1, s);
  if (int rc = mb->mark(s)) return rc;
  double h_objv[PSG_FTRL_MAX_MODELS];
  HIP_TRY(hipMemcpyAsync(mb->h_small + 2, mb->d_small + 2, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h_objv, mb->b[B_R_OBJV].p, 8 * (size_t)m, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (mb->h_small[2]) {  // as psg_mb_gradient: localize again
    mb->state = S_UNIQ;
    return fail(PSG_ERR_UNSORTED, "%llu key pairs of the dictionary not strictly increasing",
                mb->h_small[2]);
  }
  if (objv) memcpy(objv, h_objv, 8 * (size_t)m);
  if (grad_dev) *grad_dev = mb->at<double>(B_R_GRAD);
  mb->rows_m = m;
  return PSG_OK;
}

int psg_mb_rows_labels(psg_minibatch* mb, const double** y_dev, const double** xw_dev, int* m) {
  if (!mb) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state < S_LOCAL || mb->rows_m == 0)
    return fail(PSG_ERR_ARG, "psg_mb_rows_labels before psg_mb_gradient_rows");
  if (y_dev) *y_dev = mb->at<double>(B_Y);
  if (xw_dev) *xw_dev = mb->at<double>(B_R_XW);
  if (m) *m = mb->rows_m;
  return PSG_OK;
}

int psg_mb_rows_read(psg_minibatch* mb, int what, void* out, size_t cap_bytes, size_t* n_out) {
  if (!mb || !n_out) return fail(PSG_ERR_ARG, "null argument");
  *n_out = 0;
  if (what >= PSG_MB_ROWS_DARLING_DUAL)  // the multi-model Darling state (psg_darling_rows.hip)
    return psg::darling_rows_read(mb, what, out, cap_bytes, n_out);
  if (mb->state < S_LOCAL || mb->rows_m == 0)
    return fail(PSG_ERR_ARG, "psg_mb_rows_read before psg_mb_gradient_rows");
  int id;
  size_t n = mb->rows * (size_t)mb->rows_m;
  switch (what) {
    case PSG_MB_ROWS_XW: id = B_R_XW; break;
    case PSG_MB_ROWS_TAU: id = B_R_TAU; break;
    case PSG_MB_ROWS_LOSS: id = B_R_LOSS; break;
    case PSG_MB_ROWS_GRAD: id = B_R_GRAD; n = mb->ndict * (size_t)mb->rows_m; break;
    default: return fail(PSG_ERR_ARG, "psg_mb_rows_read: array %d", what);
  }
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;
  *n_out = n;
  if (8 * n > cap_bytes)
    return fail(PSG_ERR_SIZE, "psg_mb_rows_read: array %d holds %zu bytes, room for %zu", what,
                8 * n, cap_bytes);
  if (n == 0) return PSG_OK;
  if (!out) return fail(PSG_ERR_ARG, "null output");
  HIP_TRY(hipMemcpy(out, mb->b[id].p, 8 * n, hipMemcpyDeviceToHost));
  return PSG_OK;
}

}  // extern "C"
