// psg_ftrl_rows.hip -- m FTRL models per key in one table (psg_ftrl_rows.h):
// setValue (ftrl_model.h:80-112) for every (key, model j) with model j's
// parameters, pos / neg added once per key.  Column j of the result is bit
// for bit what psg_ftrl.hip gives for model j's setting: the same operations
// in the same order, in f64 (the library is built with -ffp-contract=off).
//
// Work split: a group of G lanes (the power of two >= m) owns one key, lane j
// of the group model j; a wave holds 64 / G keys.  The group's first lane
// probes and claims the key's slot (a pull's whole group probes: every lane
// reads the same address, one broadcast read) and the row id goes to the
// group by a shuffle, as do the key's old counts, which the first lane reads
// and updates.  The fresh keys of a wave take their row ids from one integer
// atomic.  The two grad_norm values are the same in every lane of a group
// (they are computed where they are used: the lanes run in lockstep, so
// "once per key" costs what once per lane does); grad, w and
// z are read and written as the contiguous 8 m bytes of the key's row.  The
// per-model nnz deltas fold across the wave's groups by shuffles, across the
// workgroup's waves through LDS, and leave by integer atomics on one of
// kFtrlmSlots counter lines.  No float atomics.
//
// Checkpoint and restore are further down: the import
// kernels, which walk the index one lane per key and take a workgroup's row
// ids from one atomic, and the whole-state export (flag scan over the index,
// sort by key, row gather by groups of G lanes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psg_ftrl_find.h"
#include "psg_ftrl_rows.h"
#include "psg_sort.h"

namespace psg {

namespace {

// The slot of `key` (!= 0), claimed if absent (*fresh); null only when every
// slot of the index is taken by other keys.
__device__ __forceinline__ FtrlmSlot* ftrlm_claim(const FtrlmTable& T, uint64_t key, bool* fresh) {
  *fresh = false;
  uint64_t b = fmix64(key) & T.mask;
  for (uint64_t probe = 0; probe <= T.mask; ++probe) {
    FtrlmSlot* s = &T.idx[b];
    uint64_t k = key_load(&s->key);
    if (k == 0) {
      k = atomicCAS((unsigned long long*)&s->key, 0ull, (unsigned long long)key);
      if (k == 0) {
        *fresh = true;
        return s;
      }
    }
    if (k == key) return s;
    b = (b + 1) & T.mask;
  }
  return nullptr;
}

__device__ __forceinline__ double grad_norm(uint64_t pos, uint64_t neg) {  // ftrl_model.h:60-63
  const double p = (double)pos, n = (double)neg;
  const double all = p + n;
  return all == 0 ? 0 : sqrt(p * n / all);
}

__device__ __forceinline__ double soft_thresholding(double x, double l1, double l2) {
  if (x > 0) {
    return x > l1 ? (x - l1) / l2 : 0;
  } else {
    return x < -l1 ? (x + l1) / l2 : 0;
  }
}

// keys strictly increasing?  As psg_ftrl.hip's check, on this model's head.
__global__ __launch_bounds__(256) void ftrlm_check_kernel(const uint64_t* __restrict__ keys,
                                                          uint64_t n,
                                                          FtrlmHead* __restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x + 1;
  if (i < n && keys[i - 1] >= keys[i]) {
    atomicAdd(&head->verdict, 1ull);
    atomicAdd(&head->err, 1ull);
  }
}

// the verdict word cleared by a kernel (not a memset node: the push may be
// captured into a graph)
__global__ void ftrlm_clear_kernel(unsigned long long* word) { *word = 0; }

__global__ __launch_bounds__(256) void ftrlm_update_kernel(FtrlmTable T,
                                                           const uint64_t* __restrict__ keys,
                                                           const uint32_t* __restrict__ pos,
                                                           const uint32_t* __restrict__ neg,
                                                           const double* __restrict__ grad,
                                                           uint64_t n) {
  FtrlmHead* head = T.head;
  __shared__ int part[4][kFtrlmMax];
  if (head->verdict) return;  // the message is rejected whole (workgroup-uniform)
  const uint32_t lane = threadIdx.x & 63u, G = 1u << T.gs, j = lane & (G - 1), m = T.m;
  const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> T.gs;
  const bool in = i < n, leader = in && j == 0;
  const uint64_t key = in ? keys[i] : 0;
  uint64_t row = kFtrlmNoRow;
  FtrlmSlot* slot = nullptr;
  bool fresh = false;
  if (leader) {
    if (key == 0) {  // at most one group of the launch: the keys are unique
      row = 0;
      if (head->zero_present == 0) head->zero_present = 1;
    } else {
      slot = ftrlm_claim(T, key, &fresh);
      if (!slot) atomicAdd(&head->overflow, 1ull);
      else if (!fresh) row = slot->row != 0 && slot->row < T.row_cap ? slot->row : kFtrlmNoRow;
    }
  }
  // the wave's fresh keys take consecutive row ids from one atomic
  const uint64_t need = __ballot(fresh);
  if (need) {
    const int first = __ffsll((long long)need) - 1;
    unsigned long long base = 0;
    if ((int)lane == first) base = atomicAdd(&head->rows_used, (unsigned long long)__popcll(need));
    base = __shfl(base, first, 64);
    if (fresh) {
      const uint64_t r = 1 + base + (uint64_t)__popcll(need & ((1ull << lane) - 1));
      if (r < T.row_cap) {
        slot->row = r;  // the store of a fresh row starts from zeros
        row = r;
      } else {
        atomicAdd(&head->overflow, 1ull);
      }
    }
  }
  // the leader reads the key's counts and writes the new ones; the row id and
  // the old counts go to the group by shuffles
  uint64_t ep = 0, en = 0;
  if (leader && row != kFtrlmNoRow) {
    ep = T.cnt[2 * row];
    en = T.cnt[2 * row + 1];
    T.cnt[2 * row] = ep + pos[i];
    T.cnt[2 * row + 1] = en + neg[i];
  }
  const int head_lane = (int)(lane & ~(G - 1));
  row = __shfl(row, head_lane, 64);
  ep = __shfl(ep, head_lane, 64);
  en = __shfl(en, head_lane, 64);
  int d_nnz = 0;
  if (in && row != kFtrlmNoRow) {
    const double sqrt_n = grad_norm(ep, en);
    const uint64_t np = ep + pos[i], nn = en + neg[i];
    const double sqrt_n_new = grad_norm(np, nn);
    if (j < m) {
      const FtrlParam P = head->P[j];
      const uint64_t at = row * m + j;
      const double w_old = T.w[at];
      const double sigma = (sqrt_n_new - sqrt_n) / P.alpha;
      const double z = T.z[at] + (grad[i * m + j] - sigma * w_old);
      const double lambda2 = P.lambda2 + (P.beta + sqrt_n_new) / P.alpha;
      const double w = -soft_thresholding(z, P.lambda1, lambda2);
      T.w[at] = w;
      T.z[at] = z;
      if (w == 0 && w_old != 0) {  // ftrl_model.h:106-110
        d_nnz = -1;
      } else if (w != 0 && w_old == 0) {
        d_nnz = 1;
      }
    }
  }
  // model j's delta over the wave's groups, then over the workgroup's waves
  for (uint32_t s = G; s < 64; s <<= 1) d_nnz += __shfl_xor(d_nnz, (int)s, 64);
  if (lane < G) part[threadIdx.x >> 6][lane] = d_nnz;
  __syncthreads();
  if (threadIdx.x < m) {
    const long long d = (long long)part[0][threadIdx.x] + part[1][threadIdx.x] +
                        part[2][threadIdx.x] + part[3][threadIdx.x];
    if (d)  // two's complement: the slots' sum is the signed total
      __hip_atomic_fetch_add(
          &head->nnz_slots[(blockIdx.x % kFtrlmSlots) * kFtrlmMax + threadIdx.x],
          (unsigned long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// getValue (ftrl_model.h:72-78) without the insert: the w row, +0.0 if absent
__global__ __launch_bounds__(256) void ftrlm_pull_kernel(FtrlmTable T,
                                                         const uint64_t* __restrict__ keys,
                                                         uint64_t n, double* __restrict__ out) {
  const uint32_t j = threadIdx.x & ((1u << T.gs) - 1);
  const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> T.gs;
  if (i >= n || j >= T.m) return;
  const uint64_t row = ftrlm_find(T, keys[i]);
  out[i * T.m + j] = row != kFtrlmNoRow ? T.w[row * T.m + j] : 0.0;
}

__global__ __launch_bounds__(256) void ftrlm_lookup_kernel(
    FtrlmTable T, const uint64_t* __restrict__ keys, uint64_t n, uint64_t* __restrict__ pos,
    uint64_t* __restrict__ neg, double* __restrict__ w, double* __restrict__ z,
    uint8_t* __restrict__ found) {
  const uint32_t j = threadIdx.x & ((1u << T.gs) - 1);
  const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> T.gs;
  if (i >= n || j >= T.m) return;
  const uint64_t row = ftrlm_find(T, keys[i]);
  const bool hit = row != kFtrlmNoRow;
  if (j == 0) {
    if (pos) pos[i] = hit ? T.cnt[2 * row] : 0;
    if (neg) neg[i] = hit ? T.cnt[2 * row + 1] : 0;
    if (found) found[i] = hit ? 1 : 0;
  }
  if (w) w[i * T.m + j] = hit ? T.w[row * T.m + j] : 0.0;
  if (z) z[i * T.m + j] = hit ? T.z[row * T.m + j] : 0.0;
}

// one lane per slot of the old index: the key is claimed in the new one and
// keeps its row
__global__ __launch_bounds__(256) void ftrlm_rehash_kernel(FtrlmTable from, FtrlmTable to) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > from.mask) return;
  const FtrlmSlot o = from.idx[i];
  if (!o.key) return;
  bool fresh;
  FtrlmSlot* s = ftrlm_claim(to, o.key, &fresh);
  if (!s) {
    atomicAdd(&to.head->overflow, 1ull);
    return;
  }
  s->row = o.row;
}

// nnz_res[j] = the sum of model j's counter slots: lane t sums every eighth
// slot of model t % 32 (integers: any order)
__global__ __launch_bounds__(256) void ftrlm_count_kernel(FtrlmHead* __restrict__ head) {
  __shared__ long long s[256];
  const uint32_t j = threadIdx.x & 31u;
  long long a = 0;
  for (uint32_t k = threadIdx.x >> 5; k < (uint32_t)kFtrlmSlots; k += 8)
    a += (long long)head->nnz_slots[k * kFtrlmMax + j];
  s[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x < 32) {
    for (int k = 1; k < 8; ++k) a += s[threadIdx.x + 32 * k];
    head->nnz_res[threadIdx.x] = (unsigned long long)a;
  }
}

// The two norms of every model.  Workgroup g takes the rows [g * per,
// (g + 1) * per) of the rows in use; lane t adds column t % G of every
// (256 / G)-th row of them one after the other, and the lanes of one column
// fold by a fixed tree.  The order depends on the rows' ids, which the claim
// order of the pushes decides: the same model can give sums that differ in
// their last bits from run to run (within the bound of include/psg.h).
__device__ __forceinline__ void column_tree(double* s1, double* s2, uint32_t G) {
  __syncthreads();
  for (uint32_t h = 128; h >= G; h >>= 1) {
    if (threadIdx.x < h) {
      s1[threadIdx.x] += s1[threadIdx.x + h];
      s2[threadIdx.x] += s2[threadIdx.x + h];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ftrlm_norm_kernel(FtrlmTable T) {
  __shared__ double s1[256], s2[256];
  const uint32_t G = 1u << T.gs, j = threadIdx.x & (G - 1), m = T.m;
  const uint64_t used = T.head->rows_used + 1;  // row 0 holds zeros until key 0 is pushed
  const uint64_t nrows = used < T.row_cap ? used : T.row_cap;
  const uint64_t per = (nrows + gridDim.x - 1) / gridDim.x;
  const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < nrows ? lo + per : nrows;
  double a = 0, q = 0;
  if (j < m)
    for (uint64_t row = lo + (threadIdx.x >> T.gs); row < hi; row += 256u >> T.gs) {
      const double w = T.w[row * m + j];
      a += fabs(w);
      q += w * w;
    }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = q;
  column_tree(s1, s2, G);
  if (threadIdx.x < m) {
    T.head->partial[2 * (blockIdx.x * kFtrlmMax + threadIdx.x)] = s1[threadIdx.x];
    T.head->partial[2 * (blockIdx.x * kFtrlmMax + threadIdx.x) + 1] = s2[threadIdx.x];
  }
}

__global__ __launch_bounds__(256) void ftrlm_norm_final_kernel(FtrlmHead* __restrict__ head,
                                                               uint32_t nparts, uint32_t m,
                                                               uint32_t gs) {
  __shared__ double s1[256], s2[256];
  const uint32_t G = 1u << gs, j = threadIdx.x & (G - 1);
  double a = 0, q = 0;
  if (j < m)
    for (uint32_t p = threadIdx.x >> gs; p < nparts; p += 256u >> gs) {
      a += head->partial[2 * (p * kFtrlmMax + j)];
      q += head->partial[2 * (p * kFtrlmMax + j) + 1];
    }
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = q;
  column_tree(s1, s2, G);
  if (threadIdx.x < m) {
    head->norm_res[2 * threadIdx.x] = s1[threadIdx.x];
    head->norm_res[2 * threadIdx.x + 1] = s2[threadIdx.x];
  }
}

// writeToFile's filter (ftrl_model.h:26-28) for model jm: lane i <= mask is an
// index slot, lane mask + 1 key 0
__global__ __launch_bounds__(256) void ftrlm_export_kernel(FtrlmTable T, uint32_t jm,
                                                           uint64_t* __restrict__ keys,
                                                           double* __restrict__ w, uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > T.mask + 1) return;
  uint64_t key = 0, row = kFtrlmNoRow;
  if (i <= T.mask) {
    const FtrlmSlot s = T.idx[i];
    key = s.key;
    if (key != 0 && s.row != 0 && s.row < T.row_cap) row = s.row;
  } else if (T.head->zero_present) {
    row = 0;
  }
  if (row == kFtrlmNoRow) return;
  const double v = T.w[row * T.m + jm];
  if (v != 0) {
    const unsigned long long at = atomicAdd(&T.head->export_n, 1ull);
    if (at < cap) {
      keys[at] = key;
      w[at] = v;
    }
  }
}

// ---- import -----------------------------------------------
constexpr uint64_t kFreshBit = 1ull << 62;  // row ids are below 2^32

// Phase 1 of both import kernels: lane t of the workgroup owns key t of its
// 256 (`in`: there is one; every lane comes here).  The row is found, or
// claimed by the update kernel's walk and CAS; the workgroup's fresh keys are
// counted by a scan and take consecutive row ids from ONE integer atomic on
// head->rows_used.  (One atomic per wave, as the update kernel has it, is what
// bounds a launch of few keys per wave: every wave waits its turn on that one
// address.)  Key 0 is row 0.  Returns the row, or kFtrlmNoRow; *fresh_row: the
// row held no entry before (its store is zeros).
__device__ __forceinline__ uint64_t ftrlm_block_rows(const FtrlmTable& T, uint64_t key, bool in,
                                                     uint32_t* ws, unsigned long long* base,
                                                     bool* fresh_row) {
  FtrlmHead* head = T.head;
  uint64_t row = kFtrlmNoRow;
  FtrlmSlot* slot = nullptr;
  bool fresh = false, fresh0 = false;
  if (in) {
    if (key == 0) {  // at most one lane of the launch: the keys are unique
      row = 0;
      fresh0 = head->zero_present == 0;
      if (fresh0) head->zero_present = 1;
    } else {
      slot = ftrlm_claim(T, key, &fresh);
      if (!slot) atomicAdd(&head->overflow, 1ull);
      else if (!fresh) row = slot->row != 0 && slot->row < T.row_cap ? slot->row : kFtrlmNoRow;
    }
  }
  uint32_t total;
  const uint32_t before = block_exscan(fresh ? 1u : 0u, ws, &total);
  if (threadIdx.x == 0 && total) *base = atomicAdd(&head->rows_used, (unsigned long long)total);
  __syncthreads();
  if (fresh) {
    const uint64_t r = 1 + *base + before;
    if (r < T.row_cap) {
      slot->row = r;
      row = r;
    } else {
      atomicAdd(&head->overflow, 1ull);
    }
  }
  *fresh_row = fresh0 || (fresh && row != kFtrlmNoRow);
  return row;
}

// (w_new != 0) - (w_old != 0) with ftrl_model.h:106-110's comparisons: -0.0 is
// zero, a NaN weight is not
__device__ __forceinline__ int nnz_step(double w_new, double w_old) {
  return (w_new != 0 ? 1 : 0) - (w_old != 0 ? 1 : 0);
}

// A workgroup owns 256 entries of the image whatever m is.  Phase 1: one lane
// per key finds or claims the row (above) and stores the two counts; the row
// ids wait in LDS.  Phase 2: the workgroup walks its keys 256 / G at a time, a
// group of G lanes per key, lane j replacing w[row][j] and z[row][j]: the
// image's rows are read and the store's rows written as contiguous 8 m bytes,
// and the rows of a workgroup's fresh keys are neighbours.  Every bit is
// stored as given.  The nnz deltas leave as the update kernel's do.
__global__ __launch_bounds__(256) void ftrlm_import_kernel(FtrlmTable T,
                                                           const uint64_t* __restrict__ keys,
                                                           const uint64_t* __restrict__ pos,
                                                           const uint64_t* __restrict__ neg,
                                                           const double* __restrict__ w,
                                                           const double* __restrict__ z,
                                                           uint64_t n) {
  FtrlmHead* head = T.head;
  __shared__ int part[4][kFtrlmMax];
  __shared__ uint64_t rows[256];
  __shared__ uint32_t ws[4];
  __shared__ unsigned long long base;
  if (head->verdict) return;  // the message is rejected whole (workgroup-uniform)
  const uint32_t lane = threadIdx.x & 63u, G = 1u << T.gs, j = lane & (G - 1), m = T.m;
  const uint64_t i0 = (uint64_t)blockIdx.x * 256u, i = i0 + threadIdx.x;
  const bool in = i < n;
  bool fresh;
  const uint64_t row = ftrlm_block_rows(T, in ? keys[i] : 0, in, ws, &base, &fresh);
  if (in && row != kFtrlmNoRow) {
    T.cnt[2 * row] = pos[i];
    T.cnt[2 * row + 1] = neg[i];
  }
  rows[threadIdx.x] = row == kFtrlmNoRow ? row : row | (fresh ? kFreshBit : 0);
  __syncthreads();
  const uint32_t nkeys = (uint32_t)(n - i0 < 256u ? n - i0 : 256u);
  int d_nnz = 0;
  if (j < m)
    for (uint32_t t = threadIdx.x >> T.gs; t < nkeys; t += 256u >> T.gs) {
      const uint64_t r = rows[t];
      if (r == kFtrlmNoRow) continue;
      const uint64_t at = (r & ~kFreshBit) * m + j, from = (i0 + t) * m + j;
      const double w_old = (r & kFreshBit) ? 0.0 : T.w[at], w_new = w[from];
      T.w[at] = w_new;
      T.z[at] = z[from];
      d_nnz += nnz_step(w_new, w_old);
    }
  for (uint32_t s = G; s < 64; s <<= 1) d_nnz += __shfl_xor(d_nnz, (int)s, 64);
  if (lane < G) part[threadIdx.x >> 6][lane] = d_nnz;
  __syncthreads();
  if (threadIdx.x < m) {
    const long long d = (long long)part[0][threadIdx.x] + part[1][threadIdx.x] +
                        part[2][threadIdx.x] + part[3][threadIdx.x];
    if (d)  // two's complement: the slots' sum is the signed total
      __hip_atomic_fetch_add(
          &head->nnz_slots[(blockIdx.x % kFtrlmSlots) * kFtrlmMax + threadIdx.x],
          (unsigned long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Column jm alone, one lane per key throughout: w[row][jm] is replaced, the
// row's other columns, its z and its counts stay (zeros in a fresh row: the
// store is zeroed when it is allocated).
__global__ __launch_bounds__(256) void ftrlm_import_weights_kernel(
    FtrlmTable T, uint32_t jm, const uint64_t* __restrict__ keys, const double* __restrict__ w,
    uint64_t n) {
  FtrlmHead* head = T.head;
  __shared__ int part[4];
  __shared__ uint32_t ws[4];
  __shared__ unsigned long long base;
  if (head->verdict) return;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const bool in = i < n;
  bool fresh;
  const uint64_t row = ftrlm_block_rows(T, in ? keys[i] : 0, in, ws, &base, &fresh);
  int d_nnz = 0;
  if (in && row != kFtrlmNoRow) {
    const uint64_t at = row * T.m + jm;
    const double w_old = fresh ? 0.0 : T.w[at], w_new = w[i];
    T.w[at] = w_new;
    d_nnz = nnz_step(w_new, w_old);
  }
  for (int s = 32; s >= 1; s >>= 1) d_nnz += __shfl_xor(d_nnz, s, 64);
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = d_nnz;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long d = (long long)part[0] + part[1] + part[2] + part[3];
    if (d)
      __hip_atomic_fetch_add(&head->nnz_slots[(blockIdx.x % kFtrlmSlots) * kFtrlmMax + jm],
                             (unsigned long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- whole-state export -----------------------------------
// Element i < slots of the flag scans is an index slot, element `slots` the
// side entry (key 0, row 0).  Flagged: holds a row and lo <= key <= hi.
struct RowsFlag {
  FtrlmTable T;
  uint64_t lo, hi;
  uint32_t nslots;
  __device__ bool entry(uint32_t i, uint64_t* key, uint32_t* row) const {
    if (i < nslots) {
      const FtrlmSlot s = T.idx[i];
      *key = s.key;
      *row = (uint32_t)s.row;
      return s.key != 0 && s.row != 0 && s.row < T.row_cap && s.key >= lo && s.key <= hi;
    }
    *key = 0;
    *row = 0;
    return T.head->zero_present != 0 && lo == 0;
  }
  __device__ bool operator()(uint32_t i) const {
    uint64_t k;
    uint32_t r;
    return entry(i, &k, &r);
  }
};

// the compacted (key, row id) of the flagged elements, in slot order
struct RowsEmit {
  RowsFlag f;
  uint64_t* ckey;
  uint32_t* crow;
  uint32_t cap;
  __device__ void operator()(uint32_t i, uint32_t ex, bool flagged, uint32_t) const {
    if (!flagged || ex >= cap) return;  // ex < cap always, by the count
    uint64_t k;
    uint32_t r;
    (void)f.entry(i, &k, &r);
    ckey[ex] = k;
    crow[ex] = r;
  }
};

__global__ void ftrlm_state_init_kernel(unsigned long long* small) {
  small[0] = 0;
  small[1] = ~0ull;
  small[2] = 0;
}

// One pass over the index in flag_count_kernel's tile shape (a lane owns 8
// consecutive slots, one 128-B line): the tile's flag count for the scan, and
// orand[0] |= / orand[1] &= every flagged key, folded over the wave first.
__global__ __launch_bounds__(256) void ftrlm_state_count_kernel(
    RowsFlag f, uint32_t n, uint32_t* __restrict__ tile_sum,
    unsigned long long* __restrict__ orand) {
  __shared__ uint32_t ws[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kFlagTile + threadIdx.x * 8u;
  uint32_t c = 0;
  uint64_t o = 0, a = ~0ull;
  for (uint32_t j = 0; j < 8; ++j)
    if (i0 + j < n) {
      uint64_t k;
      uint32_t r;
      if (f.entry((uint32_t)(i0 + j), &k, &r)) {
        ++c;
        o |= k;
        a &= k;
      }
    }
  for (int s = 32; s >= 1; s >>= 1) {
    o |= __shfl_xor(o, s, 64);
    a &= __shfl_xor(a, s, 64);
  }
  if ((threadIdx.x & 63u) == 0 && (o | ~a)) {
    atomicOr(orand, (unsigned long long)o);
    atomicAnd(orand + 1, (unsigned long long)a);
  }
  uint32_t tot;
  (void)block_exscan(c, ws, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// A group of G lanes owns output entry i, the i-th key in key order.  Its
// first lane reads the sorted pair's place, the row id there and the row's
// counts; the row id goes round by shuffle and lane j copies w[row][j] and
// z[row][j]: whole rows read, whole rows of the image written.
__global__ __launch_bounds__(256) void ftrlm_state_gather_kernel(
    FtrlmTable T, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ spos,
    const uint32_t* __restrict__ crow, uint32_t n, uint64_t* __restrict__ keys,
    uint64_t* __restrict__ pos, uint64_t* __restrict__ neg, double* __restrict__ w,
    double* __restrict__ z) {
  const uint32_t lane = threadIdx.x & 63u, G = 1u << T.gs, j = lane & (G - 1), m = T.m;
  const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> T.gs;
  const bool in = i < n;
  uint64_t row = kFtrlmNoRow;
  if (in && j == 0) {
    const uint32_t at = spos[i];
    if (at < n && crow[at] < T.row_cap) row = crow[at];  // always: a permutation, a live row
    if (row != kFtrlmNoRow) {
      if (keys) keys[i] = skey[i];
      if (pos) pos[i] = T.cnt[2 * row];
      if (neg) neg[i] = T.cnt[2 * row + 1];
    }
  }
  row = __shfl(row, (int)(lane & ~(G - 1)), 64);
  if (in && j < m && row != kFtrlmNoRow) {
    if (w) w[i * m + j] = T.w[row * m + j];
    if (z) z[i * m + j] = T.z[row * m + j];
  }
}

// the blocks of launch_ftrlm_state's work area for n entries
struct RowsWork {
  size_t ckey, key_a, key_b, crow, pos_a, pos_b, counts, dtotal, end;
  explicit RowsWork(uint64_t n) {
    const size_t k8 = (size_t)(8 * n + 255) & ~(size_t)255, k4 = (size_t)(4 * n + 255) & ~(size_t)255;
    ckey = 0;
    key_a = ckey + k8;
    key_b = key_a + k8;
    crow = key_b + k8;
    pos_a = crow + k4;
    pos_b = pos_a + k4;
    counts = pos_b + k4;
    dtotal = counts + 4 * 256 * (size_t)blocks_of(n, kSortTile);
    end = dtotal + 4 * 256;
  }
};

// lanes per key -> keys per workgroup of 256
inline uint32_t group_blocks(const FtrlmTable& T, uint64_t n) { return blocks_of(n, 256u >> T.gs); }

}  // namespace

hipError_t launch_ftrlm_push(const FtrlmTable& T, const uint64_t* keys, const uint32_t* pos,
                             const uint32_t* neg, const double* grad, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ftrlm_clear_kernel, dim3(1), dim3(1), 0, s, &T.head->verdict);
  if (n > 1)
    hipLaunchKernelGGL(ftrlm_check_kernel, dim3(blocks_of(n - 1, 256)), dim3(256), 0, s, keys, n,
                       T.head);
  hipLaunchKernelGGL(ftrlm_update_kernel, dim3(group_blocks(T, n)), dim3(256), 0, s, T, keys, pos,
                     neg, grad, n);
  return hipGetLastError();
}

hipError_t launch_ftrlm_pull(const FtrlmTable& T, const uint64_t* keys, uint64_t n, double* out,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ftrlm_pull_kernel, dim3(group_blocks(T, n)), dim3(256), 0, s, T, keys, n, out);
  return hipGetLastError();
}

hipError_t launch_ftrlm_lookup(const FtrlmTable& T, const uint64_t* keys, uint64_t n,
                               uint64_t* pos, uint64_t* neg, double* w, double* z, uint8_t* found,
                               hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ftrlm_lookup_kernel, dim3(group_blocks(T, n)), dim3(256), 0, s, T, keys, n,
                     pos, neg, w, z, found);
  return hipGetLastError();
}

hipError_t launch_ftrlm_rehash(const FtrlmTable& from, const FtrlmTable& to, hipStream_t s) {
  hipLaunchKernelGGL(ftrlm_rehash_kernel, dim3(blocks_of(from.mask + 1, 256)), dim3(256), 0, s,
                     from, to);
  return hipGetLastError();
}

hipError_t launch_ftrlm_count(const FtrlmTable& T, hipStream_t s) {
  hipLaunchKernelGGL(ftrlm_count_kernel, dim3(1), dim3(256), 0, s, T.head);
  return hipGetLastError();
}

hipError_t launch_ftrlm_status(const FtrlmTable& T, hipStream_t s) {
  hipLaunchKernelGGL(ftrlm_count_kernel, dim3(1), dim3(256), 0, s, T.head);
  hipLaunchKernelGGL(ftrlm_norm_kernel, dim3(kFtrlmParts), dim3(256), 0, s, T);
  hipLaunchKernelGGL(ftrlm_norm_final_kernel, dim3(1), dim3(256), 0, s, T.head,
                     (uint32_t)kFtrlmParts, T.m, T.gs);
  return hipGetLastError();
}

hipError_t launch_ftrlm_export(const FtrlmTable& T, int j, uint64_t* keys, double* w, uint64_t cap,
                               hipStream_t s) {
  hipLaunchKernelGGL(ftrlm_clear_kernel, dim3(1), dim3(1), 0, s, &T.head->export_n);
  hipLaunchKernelGGL(ftrlm_export_kernel, dim3(blocks_of(T.mask + 2, 256)), dim3(256), 0, s, T,
                     (uint32_t)j, keys, w, cap);
  return hipGetLastError();
}

hipError_t launch_ftrlm_import(const FtrlmTable& T, const uint64_t* keys, const uint64_t* pos,
                               const uint64_t* neg, const double* w, const double* z, uint64_t n,
                               hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ftrlm_clear_kernel, dim3(1), dim3(1), 0, s, &T.head->verdict);
  if (n > 1)
    hipLaunchKernelGGL(ftrlm_check_kernel, dim3(blocks_of(n - 1, 256)), dim3(256), 0, s, keys, n,
                       T.head);
  hipLaunchKernelGGL(ftrlm_import_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, T, keys, pos,
                     neg, w, z, n);
  return hipGetLastError();
}

hipError_t launch_ftrlm_import_weights(const FtrlmTable& T, int j, const uint64_t* keys,
                                       const double* w, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ftrlm_clear_kernel, dim3(1), dim3(1), 0, s, &T.head->verdict);
  if (n > 1)
    hipLaunchKernelGGL(ftrlm_check_kernel, dim3(blocks_of(n - 1, 256)), dim3(256), 0, s, keys, n,
                       T.head);
  hipLaunchKernelGGL(ftrlm_import_weights_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, T,
                     (uint32_t)j, keys, w, n);
  return hipGetLastError();
}

size_t ftrlm_state_count_words(const FtrlmTable& T) { return blocks_of(T.mask + 2, kFlagTile); }

int launch_ftrlm_state_count(const FtrlmTable& T, uint64_t lo, uint64_t hi, uint32_t* tile_sum,
                             unsigned long long* small, hipStream_t s) {
  const uint64_t nel = T.mask + 2;  // the slots and the side entry
  if (nel > 0xffffffffull)  // the sort's payload and the scans' element ids are 32 bits
    return fail(PSG_ERR_SIZE, "multi-model FTRL state export: an index of %llu slots >= 2^32 - 1",
                (unsigned long long)(nel - 1));
  const RowsFlag f{T, lo, hi, (uint32_t)(nel - 1)};
  const uint32_t nt = blocks_of(nel, kFlagTile);
  hipLaunchKernelGGL(ftrlm_state_init_kernel, dim3(1), dim3(1), 0, s, small);
  LAUNCH(ftrlm_state_count_kernel, nt, s, f, (uint32_t)nel, tile_sum, small);
  LAUNCH(row_scan_kernel, 1, s, tile_sum, nt, (uint32_t*)(small + 2));
  return launched("ftrlm state count");
}

size_t ftrlm_state_work_bytes(uint64_t n) { return RowsWork(n).end; }

int launch_ftrlm_state(const FtrlmTable& T, uint64_t lo, uint64_t hi, uint64_t n, uint64_t differ,
                       const uint32_t* tile_base, void* work, uint64_t* keys, uint64_t* pos,
                       uint64_t* neg, double* w, double* z, hipStream_t s) {
  if (n == 0) return PSG_OK;
  const uint64_t nel = T.mask + 2;
  const RowsWork W(n);
  char* base = (char*)work;
  uint64_t* ckey = (uint64_t*)(base + W.ckey);
  uint32_t* crow = (uint32_t*)(base + W.crow);
  const RowsFlag f{T, lo, hi, (uint32_t)(nel - 1)};
  const RowsEmit em{f, ckey, crow, (uint32_t)n};
  LAUNCH((flag_emit_kernel<RowsFlag, RowsEmit>), blocks_of(nel, kFlagTile), s, f, em,
         (uint32_t)nel, tile_base);
  const SortBuffers sb{(uint64_t*)(base + W.key_a), (uint64_t*)(base + W.key_b),
                       (uint32_t*)(base + W.pos_a), (uint32_t*)(base + W.pos_b),
                       (uint32_t*)(base + W.counts), (uint32_t*)(base + W.dtotal)};
  const uint64_t* skey = nullptr;
  const uint32_t* spos = nullptr;
  if (int rc = enqueue_radix_sort(ckey, (uint32_t)n, differ, sb, &skey, &spos, s)) return rc;
  LAUNCH(ftrlm_state_gather_kernel, group_blocks(T, n), s, T, skey, spos, crow, (uint32_t)n, keys,
         pos, neg, w, z);
  return launched("ftrlm state export");
}

}  // namespace psg
