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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psg_ftrl_rows.h"
#include "psg_sort.h"

namespace psg {

namespace {

__device__ __forceinline__ uint64_t fmix64(uint64_t k) {  // MurmurHash3 finaliser
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

__device__ __forceinline__ uint64_t key_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The row of `key`, or kFtrlmNoRow.  A slot whose row word is 0 was claimed
// by a key that found no row (an overflow, already counted): absent.
__device__ __forceinline__ uint64_t ftrlm_find(const FtrlmTable& T, uint64_t key) {
  if (key == 0) return T.head->zero_present ? 0 : kFtrlmNoRow;
  uint64_t b = fmix64(key) & T.mask;
  for (uint64_t probe = 0; probe <= T.mask; ++probe) {
    const FtrlmSlot s = T.idx[b];
    if (s.key == key) return s.row != 0 && s.row < T.row_cap ? s.row : kFtrlmNoRow;
    if (s.key == 0) return kFtrlmNoRow;
    b = (b + 1) & T.mask;
  }
  return kFtrlmNoRow;
}

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

}  // namespace psg
