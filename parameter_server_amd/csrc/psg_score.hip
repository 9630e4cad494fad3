// psg_score.hip -- the direct scorer: ModelEvaluation::run's inner loop
// (src/linear_method/model_evaluation.h:48-57) for a loaded minibatch against
// the resident model, with no sort, unique pass, localize or dictionary:
//   re = 0;  for every entry of the row, in order:
//     if the key has an entry: re = re + w * value      (binary: re + w)
// in double (PSG_SCORE_F64) or in the reference's Real = float
// (PSG_SCORE_F32: w and value rounded to float, float multiply, float add,
// the sum widened on store).  An absent key adds nothing, not even +0.0 * v.
//
// A row's sum is one serial chain, the probes are independent random 128-B
// reads and they are the cost, so the work is split by entries: a workgroup of
// 256 lanes takes a tile of consecutive entries, whatever rows they belong to.
//
// Scalar model (score_kernel): a lane owns kScoreKpl entries of the tile
// (entry u * 256 + lane: coalesced keys and values) and requests the keys and
// then the three key words of every first bucket before it looks at any;
// later buckets are read only by the lanes that need them (ftrl_find).  The
// product goes to the tile's LDS term array, presence to an LDS bit mask (one
// ballot per wave and round, no zero term).  While the probes are in flight
// two lanes find the rows that start in the tile from the load's row_of block.
// After one barrier a lane per row that lies wholly in the tile walks its
// terms in order and stores Xw.
//
// Sweep (score_rows_kernel): phase A as above against the 16-B index slots
// gives every entry's row id (LDS); phase B, a group of G lanes (the power of
// two >= m) per entry reads w[row][0..m) contiguously, as ftrlm_pull_kernel
// does, into terms [tile][m]; phase C, a lane per (row, model).  The tile
// shrinks with m so that terms, values, row ids and mask fit kScoreLds bytes.
//
// A row cut by a tile edge (at most one starts in a tile and leaves it) or
// longer than a tile: the tiles spill those entries' terms and the mask words
// to two scratch blocks of the minibatch and note the row (cut_row[tile]); a
// second step sums them in order, one lane per (cut row, model) up to kLongRun
// entries, one wave for a longer row and all its models (64 terms per load,
// four loads ahead, laid out in LDS and added from there, a lane per model).  No float atomics, no
// partial sums.  Whether a row was cut is known on the device only, so the
// second step is always enqueued (two launches of one lane or wave per tile);
// a minibatch of one tile has no edge and pays one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "psg_ftrl_find.h"
#include "psg_minibatch.h"
#include "psg_score.h"
#include "psg_sort.h"

namespace psg {
namespace {

// Entries per lane of the scalar kernel = probes a lane keeps in flight.
// Measured: 65,536 x 64 entries against 2^22 keys.
#ifndef PSG_SCORE_KPL
#define PSG_SCORE_KPL 4  // A/B builds: 1, 2, 8
#endif
// LDS bytes of a sweep tile: what bounds the workgroups per CU (160 KB).
#ifndef PSG_SCORE_LDS
#define PSG_SCORE_LDS (24u << 10)  // A/B builds: 48 KB, 64 KB
#endif
constexpr int kScoreKpl = PSG_SCORE_KPL;
constexpr uint32_t kScoreTile = 256u * kScoreKpl;
constexpr uint32_t kScoreLds = PSG_SCORE_LDS;
constexpr int kRowsKpl = 4;  // the sweep's phase A: at most this many entries per lane
constexpr uint32_t kRowsTileMax = 256u * kRowsKpl;
constexpr uint32_t kNoCut = 0xffffffffu, kNoRow32 = 0xffffffffu;

// entries per tile of the sweep kernel: a multiple of 64 whose mask, terms,
// values and row ids fit kScoreLds
inline uint32_t rows_tile(uint32_t m, uint32_t sz) {
  const uint64_t per8 = 8ull * (m * sz + sz + 4) + 1;  // eighths of a byte per entry
  const uint32_t t = (uint32_t)(8ull * kScoreLds / per8) & ~63u;
  return std::min(kRowsTileMax, std::max(64u, t));
}
inline size_t rows_lds(uint32_t T, uint32_t m, uint32_t sz) {
  return (size_t)T / 8 + (size_t)T * m * sz + (size_t)T * sz + 4 * (size_t)T;
}

// the first row of offset[0 .. rows] with offset[row] >= x (x <= offset[rows])
__device__ __forceinline__ uint32_t first_row_at(const uint64_t* __restrict__ offset,
                                                 uint32_t rows, uint64_t x) {
  uint32_t lo = 0, hi = rows;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (offset[mid] < x) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// The same for an entry x < n, from the row that holds it (row_of[x]: the last
// row with offset[row] <= x, written by the load): three dependent loads where
// the search takes seventeen.  Empty rows that start at x come before that row;
// past a few of them the search takes over.
__device__ __forceinline__ uint32_t first_row_from(const uint64_t* __restrict__ offset,
                                                   const uint32_t* __restrict__ row_of,
                                                   uint32_t rows, uint32_t x) {
  uint32_t r = row_of[x];
  if (r >= rows) return first_row_at(offset, rows, x);  // never
  if (offset[r] < x) return r + 1;
  for (int k = 0; k < 8; ++k) {
    if (r == 0 || offset[r - 1] < x) return r;
    --r;
  }
  return first_row_at(offset, rows, x);
}

// ((0 + t[lb]) + ...) over the present entries of [lb, le), column j of terms
// [.][m]; term and mask start at the same entry (a tile's in LDS, the
// minibatch's in the spill)
template <class Real>
__device__ __forceinline__ Real ordered_sum(const Real* term, const uint64_t* mask, uint32_t lb,
                                            uint32_t le, uint32_t m, uint32_t j) {
  Real acc = 0;
  uint32_t i = lb;
  while (i < le) {
    uint64_t mk = mask[i >> 6] >> (i & 63u);
    const uint32_t stop = (i | 63u) + 1u, end = stop < le && stop != 0 ? stop : le;
    for (; i < end; ++i, mk >>= 1)
      if (mk & 1u) acc = acc + term[(size_t)i * m + j];
  }
  return acc;
}

// The tile [a, b) with its terms and mask in LDS (after the barrier) and
// edge[0 .. 1] = the rows [rb, re) that start in it: note the cut row, spill
// the entries of rows that do not lie wholly in the tile, sum the ones that do.
template <class Real>
__device__ __forceinline__ void finish_tile(const Real* term, const uint64_t* mask, uint32_t m,
                                            uint32_t a, uint32_t b, const uint32_t* edge,
                                            const uint64_t* __restrict__ offset, uint32_t rows,
                                            double* __restrict__ xw, Real* __restrict__ sterm,
                                            uint64_t* __restrict__ smask,
                                            uint32_t* __restrict__ cut_row) {
  const uint32_t rb = edge[0], re = edge[1] > rb ? edge[1] : rb;
  // [a, lead_end): the tail of a row that started in an earlier tile
  const uint64_t ob = offset[rb];
  const uint32_t lead_end = ob < b ? (uint32_t)(ob > a ? ob : a) : b;
  // [trail_begin, b): the head of the last row, if it goes on past the tile
  uint32_t trail_begin = b;
  bool cut = false;
  if (re > rb && offset[re] > b) {
    const uint64_t ot = offset[re - 1];
    cut = true;
    trail_begin = ot < b ? (uint32_t)(ot > a ? ot : a) : b;
  }
  if (threadIdx.x == 0) cut_row[blockIdx.x] = cut ? re - 1 : kNoCut;
  if (lead_end > a || trail_begin < b) {
    const uint32_t cnt = (b - a) * m;
    for (uint32_t q = threadIdx.x; q < cnt; q += 256u) {
      const uint32_t i = a + q / m;
      if (i < lead_end || i >= trail_begin) sterm[(size_t)a * m + q] = term[q];
    }
    for (uint32_t w = threadIdx.x; w < (b - a + 63u) / 64u; w += 256u) smask[a / 64u + w] = mask[w];
  }
  const uint64_t whole = (uint64_t)(re - rb - (cut ? 1u : 0u)) * m;
  for (uint64_t q = threadIdx.x; q < whole; q += 256u) {
    const uint32_t r = rb + (uint32_t)(q / m), j = (uint32_t)(q % m);
    const uint64_t o0 = offset[r], o1 = offset[r + 1];
    const uint32_t lb = o0 < a ? 0u : (uint32_t)(o0 < b ? o0 - a : b - a);
    const uint32_t le = o1 < a ? 0u : (uint32_t)(o1 < b ? o1 - a : b - a);
    xw[(size_t)r * m + j] = (double)ordered_sum(term, mask, lb, le, m, j);
  }
}

template <class Real>
__global__ __launch_bounds__(256) void score_kernel(
    FtrlTable T, const uint64_t* __restrict__ offset, const uint32_t* __restrict__ row_of,
    uint32_t rows, const uint64_t* __restrict__ index, const double* __restrict__ value, uint32_t n,
    double* __restrict__ xw, Real* __restrict__ sterm, uint64_t* __restrict__ smask,
    uint32_t* __restrict__ cut_row) {
  __shared__ Real term[kScoreTile];
  __shared__ uint64_t mask[kScoreTile / 64];
  __shared__ uint32_t edge[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t a64 = (uint64_t)blockIdx.x * kScoreTile;
  const uint32_t a = (uint32_t)a64, b = (uint32_t)(a64 + kScoreTile < n ? a64 + kScoreTile : n);
  uint64_t key[kScoreKpl], bk[kScoreKpl], k0[kScoreKpl][3];
  double v[kScoreKpl];
  bool in[kScoreKpl];
#pragma unroll
  for (int u = 0; u < kScoreKpl; ++u) {
    const uint64_t i = a64 + (uint32_t)u * 256u + tid;
    in[u] = i < b;
    key[u] = in[u] ? index[i] : 0;
    v[u] = in[u] && value ? value[i] : 1.0;
  }
#pragma unroll
  for (int u = 0; u < kScoreKpl; ++u) {
    bk[u] = fmix64(key[u]) & T.mask;
#pragma unroll
    for (int s = 0; s < 3; ++s) k0[u][s] = key[u] ? T.b[bk[u]].e[s].key : 0;
  }
  // the rows that start in the tile, found while the probes are in flight
  if (tid == 0) edge[0] = first_row_from(offset, row_of, rows, a);
  if (tid == 64) edge[1] = b == n ? rows : first_row_from(offset, row_of, rows, b);
  const FtrlEntry* e[kScoreKpl];
#pragma unroll
  for (int u = 0; u < kScoreKpl; ++u) {
    e[u] = nullptr;
    if (!in[u]) continue;
    e[u] = key[u] ? ftrl_find(T, key[u], bk[u], k0[u])
                  : (T.head->side_present ? &T.head->side : nullptr);
  }
  double w[kScoreKpl];
#pragma unroll
  for (int u = 0; u < kScoreKpl; ++u) w[u] = e[u] ? e[u]->w : 0.0;
#pragma unroll
  for (int u = 0; u < kScoreKpl; ++u) {
    const uint64_t present = __ballot(e[u] != nullptr);
    term[(uint32_t)u * 256u + tid] = value ? (Real)w[u] * (Real)v[u] : (Real)w[u];
    if (lane == 0) mask[(uint32_t)u * 4u + wave] = present;
  }
  __syncthreads();
  finish_tile<Real>(term, mask, 1u, a, b, edge, offset, rows, xw, sterm, smask, cut_row);
}

template <class Real>
__global__ __launch_bounds__(256) void score_rows_kernel(
    FtrlmTable T, uint32_t tile, const uint64_t* __restrict__ offset,
    const uint32_t* __restrict__ row_of, uint32_t rows, const uint64_t* __restrict__ index, const double* __restrict__ value, uint32_t n,
    double* __restrict__ xw, Real* __restrict__ sterm, uint64_t* __restrict__ smask,
    uint32_t* __restrict__ cut_row) {
  extern __shared__ uint64_t lds[];  // rows_lds(tile, m, sizeof(Real))
  __shared__ uint32_t edge[2];
  const uint32_t m = T.m;
  uint64_t* mask = lds;
  Real* term = (Real*)(mask + tile / 64u);
  Real* val = term + (size_t)tile * m;
  uint32_t* rowid = (uint32_t*)(val + tile);
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t a64 = (uint64_t)blockIdx.x * tile;
  const uint32_t a = (uint32_t)a64, b = (uint32_t)(a64 + tile < n ? a64 + tile : n);
  // phase A: the row id of every entry
  uint64_t key[kRowsKpl], bk[kRowsKpl];
  FtrlmSlot s0[kRowsKpl];
  bool in[kRowsKpl];
#pragma unroll
  for (int u = 0; u < kRowsKpl; ++u) {
    const uint32_t el = (uint32_t)u * 256u + tid;
    in[u] = el < tile && a64 + el < b;
    key[u] = in[u] ? index[a64 + el] : 0;
    if (in[u] && value) val[el] = (Real)value[a64 + el];
  }
#pragma unroll
  for (int u = 0; u < kRowsKpl; ++u) {
    bk[u] = fmix64(key[u]) & T.mask;
    s0[u] = key[u] ? T.idx[bk[u]] : FtrlmSlot{0, 0};
  }
  if (tid == 0) edge[0] = first_row_from(offset, row_of, rows, a);
  if (tid == 64) edge[1] = b == n ? rows : first_row_from(offset, row_of, rows, b);
#pragma unroll
  for (int u = 0; u < kRowsKpl; ++u) {
    const uint32_t el = (uint32_t)u * 256u + tid;
    if (el - lane >= tile) continue;  // the wave's 64 entries lie past the tile
    uint64_t row = kFtrlmNoRow;
    if (in[u])
      row = key[u] ? ftrlm_find_from(T, key[u], bk[u], s0[u])
                   : (T.head->zero_present ? 0 : kFtrlmNoRow);
    const uint64_t present = __ballot(row != kFtrlmNoRow);
    rowid[el] = row != kFtrlmNoRow ? (uint32_t)row : kNoRow32;
    if (lane == 0) mask[el >> 6] = present;
  }
  __syncthreads();
  // phase B: G lanes per entry read the row's m weights
  const uint32_t G = 1u << T.gs, j = tid & (G - 1), per = 256u >> T.gs, nt = b - a;
  if (j < m) {
#pragma unroll 4
    for (uint32_t el = tid >> T.gs; el < nt; el += per) {
      const uint32_t row = rowid[el];
      if (row == kNoRow32) continue;
      const Real w = (Real)T.w[(uint64_t)row * m + j];
      term[(size_t)el * m + j] = value ? w * val[el] : w;
    }
  }
  __syncthreads();
  finish_tile<Real>(term, mask, m, a, b, edge, offset, rows, xw, sterm, smask, cut_row);
}

// ---- the cut rows: item q = (tile, model) ---------------------------------
__device__ __forceinline__ bool cut_item(uint64_t q, uint32_t m,
                                         const uint32_t* __restrict__ cut_row,
                                         const uint64_t* __restrict__ offset, uint32_t rows,
                                         uint32_t n, uint32_t* r, uint32_t* lb, uint32_t* le) {
  *r = cut_row[q / m];
  if (*r >= rows) return false;  // kNoCut
  const uint64_t o0 = offset[*r], o1 = offset[*r + 1];
  *le = (uint32_t)(o1 < n ? o1 : n);
  *lb = (uint32_t)(o0 < *le ? o0 : *le);
  return true;
}

template <class Real>
__global__ __launch_bounds__(256) void score_cut_short_kernel(
    const uint32_t* __restrict__ cut_row, uint32_t ntiles, uint32_t m,
    const uint64_t* __restrict__ offset, uint32_t rows, uint32_t n,
    const Real* __restrict__ sterm, const uint64_t* __restrict__ smask, double* __restrict__ xw) {
  const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (q >= (uint64_t)ntiles * m) return;
  uint32_t r, lb, le;
  if (!cut_item(q, m, cut_row, offset, rows, n, &r, &lb, &le)) return;
  if (le - lb > kLongRun) return;  // score_cut_long_kernel's
  const uint32_t j = (uint32_t)(q % m);
  xw[(size_t)r * m + j] = (double)ordered_sum(sterm, smask, lb, le, m, j);
}

// Wave w of the launch takes the cut rows of tiles w, w + waves, ...: all m
// models of a row at once.  Lane (sub, j) = (lane >> gs, lane & (G - 1)) loads
// term[entry base + sub][j], so a load is 64 consecutive terms of the spill
// (64 >> gs entries x G models), four loads ahead; each is laid out in LDS and
// every lane adds its model's present terms from there, in entry order.
template <class Real>
__global__ __launch_bounds__(256) void score_cut_long_kernel(
    const uint32_t* __restrict__ cut_row, uint32_t ntiles, uint32_t m, uint32_t gs,
    const uint64_t* __restrict__ offset, uint32_t rows, uint32_t n,
    const Real* __restrict__ sterm, const uint64_t* __restrict__ smask, double* __restrict__ xw) {
  __shared__ Real stage_all[4][64];
  const uint32_t lane = threadIdx.x & 63u;
  Real* stage = stage_all[threadIdx.x >> 6];
  const uint32_t G = 1u << gs, j = lane & (G - 1), sub = lane >> gs, epc = 64u >> gs;
  const uint64_t epc_bits = epc == 64u ? ~0ull : (1ull << epc) - 1u;
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6); t < ntiles; t += waves) {
    uint32_t r, lb, le;
    if (!cut_item(t, 1u, cut_row, offset, rows, n, &r, &lb, &le)) continue;
    if (le - lb <= kLongRun) continue;
    Real acc = 0;
    for (uint64_t base = lb; base < le; base += 64u) {
      // bit k of win: entry base + k is present
      const uint64_t wi = base >> 6;
      const uint32_t sh = (uint32_t)(base & 63u);
      uint64_t win = smask[wi] >> sh;
      if (sh && ((uint64_t)(le - 1u) >> 6) > wi) win |= smask[wi + 1] << (64u - sh);
      if (le - base < 64u) win &= (1ull << (le - base)) - 1u;
      for (uint32_t c = 0; c < G; c += 4u) {
        Real v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
          const uint64_t i = base + (uint64_t)(c + u) * epc + sub;
          v[u] = c + u < G && i < le && j < m ? sterm[i * m + j] : (Real)0;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
          if (c + u >= G) break;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          stage[lane] = v[u];
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          uint64_t bits = (win >> ((c + u) * epc)) & epc_bits;
          while (bits) {
            acc = acc + stage[((uint32_t)__ffsll((unsigned long long)bits) - 1u) * G + j];
            bits &= bits - 1u;
          }
        }
      }
    }
    if (lane < m) xw[(size_t)r * m + lane] = (double)acc;
  }
}

// a minibatch without entries: every row is empty
__global__ __launch_bounds__(256) void score_zero_kernel(double* __restrict__ xw, uint64_t cnt) {
  const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (q < cnt) xw[q] = 0.0;
}

template <class Real>
int enqueue_score(psg_minibatch* mb, const FtrlTable* T1, const FtrlmTable* Tm, double* xw,
                  hipStream_t s) {
  const uint32_t m = Tm ? Tm->m : 1u, sz = sizeof(Real);
  const uint32_t rows = (uint32_t)mb->rows, n = (uint32_t)mb->nnz;
  const uint32_t T = Tm ? rows_tile(m, sz) : kScoreTile, ntiles = blocks_of(n, T);
  if (int rc = mb->need_all({{B_SC_TERM, (size_t)n * m * sz},
                             {B_SC_MASK, 8 * (size_t)ntiles * (T / 64u)},
                             {B_SC_CUT, 4 * (size_t)ntiles}}))
    return rc;
  const uint64_t* offset = mb->at<uint64_t>(B_OFFSET);
  const uint64_t* index = mb->at<uint64_t>(B_INDEX);
  const uint32_t* row_of = mb->at<uint32_t>(B_ROW_OF);
  const double* value = mb->binary ? nullptr : mb->at<double>(B_VALUE);
  Real* sterm = mb->at<Real>(B_SC_TERM);
  uint64_t* smask = mb->at<uint64_t>(B_SC_MASK);
  uint32_t* cut = mb->at<uint32_t>(B_SC_CUT);
  if (Tm)
    hipLaunchKernelGGL(score_rows_kernel<Real>, dim3(ntiles), dim3(256), rows_lds(T, m, sz), s,
                       *Tm, T, offset, row_of, rows, index, value, n, xw, sterm, smask, cut);
  else
    LAUNCH(score_kernel<Real>, ntiles, s, *T1, offset, row_of, rows, index, value, n, xw, sterm, smask,
           cut);
  if (ntiles > 1) {  // one tile has no edge: no row is cut
    const uint64_t items = (uint64_t)ntiles * m;
    LAUNCH(score_cut_short_kernel<Real>, blocks_of(items, 256), s, cut, ntiles, m, offset, rows, n,
           sterm, smask, xw);
    LAUNCH(score_cut_long_kernel<Real>, std::min<uint32_t>(blocks_of(ntiles, 4), kLongGrid), s,
           cut, ntiles, m, Tm ? Tm->gs : 0u, offset, rows, n, sterm, smask, xw);
  }
  return launched("score");
}

}  // namespace

int mb_score(psg_minibatch* mb, psg_ctx* c, const FtrlTable* T1, const FtrlmTable* Tm, int real,
             double* xw, hipStream_t s) {
  if (real != PSG_SCORE_F64 && real != PSG_SCORE_F32)
    return fail(PSG_ERR_ARG, "score: real %d is neither PSG_SCORE_F64 nor PSG_SCORE_F32", real);
  if (mb->ctx != c) return fail(PSG_ERR_ARG, "score: the minibatch belongs to another context");
  if (mb->state < S_LOADED) return fail(PSG_ERR_ARG, "score before psg_mb_load");
  if (Tm && mb->rows && !xw) return fail(PSG_ERR_ARG, "null argument");
  if (Tm && Tm->row_cap >= kNoRow32)
    return fail(PSG_ERR_SIZE, "score: %llu rows of the sweep >= 2^32 - 1",
                (unsigned long long)Tm->row_cap);
  HIP_TRY(hipSetDevice(mb->device));
  if (!s) s = mb->stream;
  const bool own = !xw;
  if (own) xw = mb->at<double>(B_XW);
  if (mb->rows == 0) {
    if (own) mb->xw_scored = true;
    return PSG_OK;
  }
  if (int rc = mb->order(s)) return rc;
  if (mb->nnz == 0) {
    const uint64_t cnt = (uint64_t)mb->rows * (Tm ? Tm->m : 1u);
    LAUNCH(score_zero_kernel, blocks_of(cnt, 256), s, xw, cnt);
    if (int rc = launched("score")) return rc;
  } else if (int rc = real == PSG_SCORE_F32 ? enqueue_score<float>(mb, T1, Tm, xw, s)
                                            : enqueue_score<double>(mb, T1, Tm, xw, s)) {
    return rc;
  }
  if (own) mb->xw_scored = true;
  return mb->mark(s);
}

}  // namespace psg

extern "C" size_t psg_score_tile(int m, int real) {
  const uint32_t sz = real == PSG_SCORE_F32 ? 4u : 8u;
  if (m <= 0) return psg::kScoreTile;
  return psg::rows_tile((uint32_t)std::min(m, PSG_FTRL_MAX_MODELS), sz);
}
