// psg_ftrl.hip -- the online server model: FTRLModel<uint64, double>
// (src/linear_method/ftrl_model.h, driven by src/linear_method/ftrl.cc),
// resident in HBM as a hash table keyed by the feature id.
//
// setValue (ftrl_model.h:80-112), per key of a message, in f64 and in the
// reference's operation order (the library is built with -ffp-contract=off;
// f64 divide and sqrt are correctly rounded on both sides):
//   sqrt_n     = grad_norm(e.pos, e.neg)     all = pos + neg (as double);
//                                            all == 0 ? 0 : sqrt(pos * neg / all)
//   e.pos += pos[i];  e.neg += neg[i]        (uint64: sums of uint32 pass 2^32)
//   sqrt_n_new = grad_norm(e.pos, e.neg)
//   sigma      = (sqrt_n_new - sqrt_n) / alpha
//   e.z       += grad[i] - sigma * e.w
//   lambda2    = lambda2_ + (beta + sqrt_n_new) / alpha
//   e.w        = -softThresholding(e.z, lambda1_, lambda2)   (soft_thresholding.h:7-13)
// The threshold branch returns an int 0 that becomes +0.0 and is negated: a
// thresholded weight is -0.0, an untouched one +0.0.  A NaN z fails every
// comparison and lands there too.
//
// Table (psg_internal.h): 128-B buckets of three 40-B entries, bucket =
// fmix64(key) & mask, linear probing bucket to bucket.  A slot is claimed by
// a 64-bit compare-and-swap of its key word from 0; key 0 has the side entry
// of the head block.  The keys of one message are unique (the order check
// runs ahead of the update on the same stream and the update reads its
// verdict) and messages follow each other in stream order, so an entry has
// one owner lane per launch: only the claim is atomic, the entry itself is
// read and written with plain vector loads and stores.
//
// Update kernel: one key per lane.  The kernel is written for kFtrlIlp keys
// per lane in flight (the first bucket's key words of all of them requested
// before any is looked at, then their entries); at the message sizes measured
// one key per lane wins (below).  The entry and nnz counts leave by one
// integer atomic per workgroup on one of kFtrlSlots lines picked by workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psg_internal.h"
#include "psg_sort.h"

namespace psg {

namespace {

// Keys per lane in flight (update, pull).  Measured at 131,072-key messages
// into 2^24 entries: 1 -> 26 us per message, 2 -> 30, 4 -> 40,
// 8 -> 61.  A message is only 2,048 waves, so what several keys per lane save
// in misses per lane they lose twice over in lanes: one key per lane it is.
#ifndef PSG_FTRL_ILP
#define PSG_FTRL_ILP 1  // A/B builds: 2, 4, 8
#endif
constexpr int kFtrlIlp = PSG_FTRL_ILP;

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

// The entry of `key` (!= 0), or null.  k0: the key words of bucket b, as
// read earlier in this launch (they only ever change from 0).
__device__ __forceinline__ const FtrlEntry* ftrl_find(const FtrlTable& T, uint64_t key, uint64_t b,
                                                      const uint64_t k0[3]) {
  for (int s = 0; s < 3; ++s) {
    if (k0[s] == key) return &T.b[b].e[s];
    if (k0[s] == 0) return nullptr;
  }
  for (uint64_t probe = 0; probe < T.mask; ++probe) {
    b = (b + 1) & T.mask;
    for (int s = 0; s < 3; ++s) {
      const uint64_t k = T.b[b].e[s].key;
      if (k == key) return &T.b[b].e[s];
      if (k == 0) return nullptr;
    }
  }
  return nullptr;
}

// The entry of `key` (!= 0), claimed if absent (*fresh); null only when every
// slot of the table is taken by other keys.
__device__ __forceinline__ FtrlEntry* ftrl_claim(const FtrlTable& T, uint64_t key, uint64_t b,
                                                 const uint64_t k0[3], bool* fresh) {
  *fresh = false;
  for (uint64_t probe = 0; probe <= T.mask; ++probe) {
    for (int s = 0; s < 3; ++s) {
      FtrlEntry* e = &T.b[b].e[s];
      uint64_t k = probe == 0 ? k0[s] : key_load(&e->key);
      if (k == 0) {
        k = atomicCAS((unsigned long long*)&e->key, 0ull, (unsigned long long)key);
        if (k == 0) {
          *fresh = true;
          return e;
        }
      }
      if (k == key) return e;
    }
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

__device__ __forceinline__ long long wave_sum(long long v) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// keys strictly increasing?  Every violation counts in head->verdict (zeroed
// before the message) and in head->err (until reported).
__global__ __launch_bounds__(256) void ftrl_check_kernel(const uint64_t* __restrict__ keys,
                                                         uint64_t n, FtrlHead* __restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x + 1;
  if (i < n && keys[i - 1] >= keys[i]) {
    atomicAdd(&head->verdict, 1ull);
    atomicAdd(&head->err, 1ull);
  }
}

__global__ __launch_bounds__(256) void ftrl_update_kernel(FtrlTable T,
                                                          const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ pos,
                                                          const uint32_t* __restrict__ neg,
                                                          const double* __restrict__ grad,
                                                          uint64_t n, FtrlParam P) {
  FtrlHead* head = T.head;
  if (head->verdict) return;  // the message is rejected whole
  const uint64_t i0 = (uint64_t)blockIdx.x * (256u * kFtrlIlp) + threadIdx.x;
  uint64_t key[kFtrlIlp], b[kFtrlIlp], k0[kFtrlIlp][3];
  bool in[kFtrlIlp];
#pragma unroll
  for (int j = 0; j < kFtrlIlp; ++j) {
    const uint64_t i = i0 + (uint64_t)j * 256u;
    in[j] = i < n;
    key[j] = in[j] ? keys[i] : 0;
    b[j] = fmix64(key[j]) & T.mask;
  }
#pragma unroll
  for (int j = 0; j < kFtrlIlp; ++j)
#pragma unroll
    for (int s = 0; s < 3; ++s) k0[j][s] = in[j] && key[j] ? T.b[b[j]].e[s].key : 0;
  FtrlEntry* e[kFtrlIlp];
  long long d_entries = 0, d_nnz = 0;
#pragma unroll
  for (int j = 0; j < kFtrlIlp; ++j) {
    e[j] = nullptr;
    if (!in[j]) continue;
    bool fresh;
    if (key[j] == 0) {  // at most one lane of the launch: the keys are unique
      e[j] = &head->side;
      fresh = head->side_present == 0;
      if (fresh) head->side_present = 1;
    } else {
      e[j] = ftrl_claim(T, key[j], b[j], k0[j], &fresh);
      if (!e[j]) atomicAdd(&head->overflow, 1ull);
    }
    d_entries += fresh ? 1 : 0;
  }
  uint64_t ep[kFtrlIlp], en[kFtrlIlp];
  double ew[kFtrlIlp], ez[kFtrlIlp];
#pragma unroll
  for (int j = 0; j < kFtrlIlp; ++j) {
    if (!e[j]) continue;
    ep[j] = e[j]->pos;
    en[j] = e[j]->neg;
    ew[j] = e[j]->w;
    ez[j] = e[j]->z;
  }
#pragma unroll
  for (int j = 0; j < kFtrlIlp; ++j) {
    if (!e[j]) continue;
    const uint64_t i = i0 + (uint64_t)j * 256u;
    const double sqrt_n = grad_norm(ep[j], en[j]);
    const uint64_t np = ep[j] + pos[i], nn = en[j] + neg[i];
    const double sqrt_n_new = grad_norm(np, nn);
    const double sigma = (sqrt_n_new - sqrt_n) / P.alpha;
    const double z = ez[j] + (grad[i] - sigma * ew[j]);
    const double lambda2 = P.lambda2 + (P.beta + sqrt_n_new) / P.alpha;
    const double w_old = ew[j];
    const double w = -soft_thresholding(z, P.lambda1, lambda2);
    e[j]->pos = np;
    e[j]->neg = nn;
    e[j]->w = w;
    e[j]->z = z;
    if (w == 0 && w_old != 0) {  // ftrl_model.h:106-110
      --d_nnz;
    } else if (w != 0 && w_old == 0) {
      ++d_nnz;
    }
  }
  d_entries = wave_sum(d_entries);
  d_nnz = wave_sum(d_nnz);
  __shared__ long long part[4][2];
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = d_entries;
    part[threadIdx.x >> 6][1] = d_nnz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      d_entries += part[i][0];
      d_nnz += part[i][1];
    }
    unsigned long long* slot = head->slots + (blockIdx.x % kFtrlSlots) * 8;
    if (d_entries)
      __hip_atomic_fetch_add(slot, (unsigned long long)d_entries, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    if (d_nnz)  // two's complement: the slots' sum is the signed total
      __hip_atomic_fetch_add(slot + 1, (unsigned long long)d_nnz, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

// getValue (ftrl_model.h:72-78) without the insert: +0.0 for an absent key
__global__ __launch_bounds__(256) void ftrl_pull_kernel(FtrlTable T,
                                                        const uint64_t* __restrict__ keys,
                                                        uint64_t n, double* __restrict__ out) {
  const uint64_t i0 = (uint64_t)blockIdx.x * (256u * kFtrlIlp) + threadIdx.x;
  uint64_t key[kFtrlIlp], b[kFtrlIlp], k0[kFtrlIlp][3];
  bool in[kFtrlIlp];
#pragma unroll
  for (int j = 0; j < kFtrlIlp; ++j) {
    const uint64_t i = i0 + (uint64_t)j * 256u;
    in[j] = i < n;
    key[j] = in[j] ? keys[i] : 0;
    b[j] = fmix64(key[j]) & T.mask;
  }
#pragma unroll
  for (int j = 0; j < kFtrlIlp; ++j)
#pragma unroll
    for (int s = 0; s < 3; ++s) k0[j][s] = in[j] && key[j] ? T.b[b[j]].e[s].key : 0;
#pragma unroll
  for (int j = 0; j < kFtrlIlp; ++j) {
    if (!in[j]) continue;
    const FtrlEntry* e = key[j] ? ftrl_find(T, key[j], b[j], k0[j])
                                : (T.head->side_present ? &T.head->side : nullptr);
    out[i0 + (uint64_t)j * 256u] = e ? e->w : 0.0;
  }
}

__global__ __launch_bounds__(256) void ftrl_lookup_kernel(FtrlTable T,
                                                          const uint64_t* __restrict__ keys,
                                                          uint64_t n, uint64_t* __restrict__ pos,
                                                          uint64_t* __restrict__ neg,
                                                          double* __restrict__ w,
                                                          double* __restrict__ z,
                                                          uint8_t* __restrict__ found) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i], b = fmix64(key) & T.mask;
  const FtrlEntry* e;
  if (key) {
    uint64_t k0[3];
    for (int s = 0; s < 3; ++s) k0[s] = T.b[b].e[s].key;
    e = ftrl_find(T, key, b, k0);
  } else {
    e = T.head->side_present ? &T.head->side : nullptr;
  }
  if (pos) pos[i] = e ? e->pos : 0;
  if (neg) neg[i] = e ? e->neg : 0;
  if (w) w[i] = e ? e->w : 0.0;
  if (z) z[i] = e ? e->z : 0.0;
  if (found) found[i] = e ? 1 : 0;
}

// one lane per slot of the old table
__global__ __launch_bounds__(256) void ftrl_rehash_kernel(FtrlTable from, FtrlTable to) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= 3 * (from.mask + 1)) return;
  const FtrlEntry* o = &from.b[i / 3].e[i % 3];
  const uint64_t key = o->key;
  if (!key) return;
  const uint64_t b = fmix64(key) & to.mask;
  uint64_t k0[3];
  for (int s = 0; s < 3; ++s) k0[s] = key_load(&to.b[b].e[s].key);
  bool fresh;
  FtrlEntry* e = ftrl_claim(to, key, b, k0, &fresh);
  if (!e) {
    atomicAdd(&to.head->overflow, 1ull);
    return;
  }
  e->pos = o->pos;
  e->neg = o->neg;
  e->w = o->w;
  e->z = o->z;
}

__global__ __launch_bounds__(kFtrlSlots) void ftrl_count_kernel(FtrlHead* __restrict__ head) {
  long long a = (long long)head->slots[threadIdx.x * 8];
  long long c = (long long)head->slots[threadIdx.x * 8 + 1];
  a = wave_sum(a);
  c = wave_sum(c);
  __shared__ long long part[kFtrlSlots / 64][2];
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = a;
    part[threadIdx.x >> 6][1] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kFtrlSlots / 64; ++i) {
      a += part[i][0];
      c += part[i][1];
    }
    head->res[0] = (unsigned long long)a;
    head->res[1] = (unsigned long long)c;
  }
}

// The two norms by a reduction whose order depends on the table alone:
// workgroup g sums buckets [g * per, (g + 1) * per), lane t of it buckets
// t, t + 256, ... of that range one after the other; the 256 lane sums fold
// by a fixed tree.  Free slots hold w = +0.0 and add nothing.
__device__ __forceinline__ void block_tree(double* s1, double* s2, double& a, double& q) {
  s1[threadIdx.x] = a;
  s2[threadIdx.x] = q;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      s1[threadIdx.x] += s1[threadIdx.x + h];
      s2[threadIdx.x] += s2[threadIdx.x + h];
    }
    __syncthreads();
  }
  a = s1[0];
  q = s2[0];
}

__global__ __launch_bounds__(256) void ftrl_norm_kernel(FtrlTable T, uint64_t per) {
  __shared__ double s1[256], s2[256];
  const uint64_t nb = T.mask + 1;
  const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < nb ? lo + per : nb;
  double a = 0, q = 0;
  for (uint64_t b = lo + threadIdx.x; b < hi; b += 256)
    for (int s = 0; s < 3; ++s) {
      const double w = T.b[b].e[s].w;
      a += fabs(w);
      q += w * w;
    }
  block_tree(s1, s2, a, q);
  if (threadIdx.x == 0) {
    T.head->partial[2 * blockIdx.x] = a;
    T.head->partial[2 * blockIdx.x + 1] = q;
  }
}

__global__ __launch_bounds__(256) void ftrl_norm_final_kernel(FtrlHead* __restrict__ head,
                                                              uint32_t nparts) {
  __shared__ double s1[256], s2[256];
  double a = 0, q = 0;
  for (uint32_t p = threadIdx.x; p < nparts; p += 256) {
    a += head->partial[2 * p];
    q += head->partial[2 * p + 1];
  }
  block_tree(s1, s2, a, q);
  if (threadIdx.x == 0) {
    const double w = head->side_present ? head->side.w : 0.0;
    a += fabs(w);
    q += w * w;
    head->res[2] = (unsigned long long)__double_as_longlong(a);
    head->res[3] = (unsigned long long)__double_as_longlong(q);
  }
}

// writeToFile's filter (ftrl_model.h:26-28): lane i < 3 * buckets is a table
// slot, lane 3 * buckets the side entry
__global__ __launch_bounds__(256) void ftrl_export_kernel(FtrlTable T, uint64_t* __restrict__ keys,
                                                          double* __restrict__ w, uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t nslots = 3 * (T.mask + 1);
  if (i > nslots) return;
  const FtrlEntry* e = i < nslots ? &T.b[i / 3].e[i % 3] : &T.head->side;
  const bool used = i < nslots ? e->key != 0 : T.head->side_present != 0;
  if (!used) return;
  const double v = e->w;
  if (v != 0) {
    const unsigned long long at = atomicAdd(&T.head->res[4], 1ull);
    if (at < cap) {
      keys[at] = e->key;
      w[at] = v;
    }
  }
}

// ---- whole-entry import -----------------------------------------------------
// Upsert of (key, pos, neg, w, z), one key per lane: the update kernel's
// bucket walk and claim, then the entry replaced by plain stores (the order
// check ran ahead on the same stream: one owner lane per entry).  pos, neg, z
// null: the weights-only form, the entry becomes (0, 0, w, +0.0).  nnz moves
// by (w_new != 0) - (w_old != 0) with ftrl_model.h:106-110's comparisons:
// -0.0 is zero, a NaN weight is not.
__global__ __launch_bounds__(256) void ftrl_import_kernel(FtrlTable T,
                                                          const uint64_t* __restrict__ keys,
                                                          const uint64_t* __restrict__ pos,
                                                          const uint64_t* __restrict__ neg,
                                                          const double* __restrict__ w,
                                                          const double* __restrict__ z,
                                                          uint64_t n) {
  FtrlHead* head = T.head;
  if (head->verdict) return;  // the message is rejected whole
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  long long d_entries = 0, d_nnz = 0;
  if (i < n) {
    const uint64_t key = keys[i];
    FtrlEntry* e;
    bool fresh;
    if (key == 0) {  // at most one lane of the launch: the keys are unique
      e = &head->side;
      fresh = head->side_present == 0;
      if (fresh) head->side_present = 1;
    } else {
      const uint64_t b = fmix64(key) & T.mask;
      uint64_t k0[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) k0[s] = T.b[b].e[s].key;
      e = ftrl_claim(T, key, b, k0, &fresh);
      if (!e) atomicAdd(&head->overflow, 1ull);
    }
    if (e) {
      const double w_old = fresh ? 0.0 : e->w;
      const double w_new = w[i];
      e->pos = pos ? pos[i] : 0;
      e->neg = neg ? neg[i] : 0;
      e->w = w_new;
      e->z = z ? z[i] : 0.0;
      d_entries = fresh ? 1 : 0;
      d_nnz = (w_new != 0 ? 1 : 0) - (w_old != 0 ? 1 : 0);
    }
  }
  d_entries = wave_sum(d_entries);
  d_nnz = wave_sum(d_nnz);
  __shared__ long long part[4][2];
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = d_entries;
    part[threadIdx.x >> 6][1] = d_nnz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < 4; ++j) {
      d_entries += part[j][0];
      d_nnz += part[j][1];
    }
    unsigned long long* slot = head->slots + (blockIdx.x % kFtrlSlots) * 8;
    if (d_entries)
      __hip_atomic_fetch_add(slot, (unsigned long long)d_entries, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    if (d_nnz)  // two's complement: the slots' sum is the signed total
      __hip_atomic_fetch_add(slot + 1, (unsigned long long)d_nnz, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- whole-state export -----------------------------------------------------
// Element i < 3 * buckets of the flag scans is a table slot, element
// 3 * buckets the side entry (key 0).  Flagged: occupied and lo <= key <= hi.
struct StateFlag {
  FtrlTable T;
  uint64_t lo, hi;
  uint32_t nslots;
  __device__ bool key_of(uint32_t i, uint64_t* key) const {
    if (i < nslots) {
      *key = T.b[i / 3].e[i % 3].key;
      return *key != 0;
    }
    *key = 0;
    return T.head->side_present != 0;
  }
  __device__ bool operator()(uint32_t i) const {
    uint64_t k;
    return key_of(i, &k) && k >= lo && k <= hi;
  }
};

// the compacted (key, slot id) of the flagged slots, in slot order
struct StateEmit {
  StateFlag f;
  uint64_t* ckey;
  uint32_t* cslot;
  uint32_t cap;
  __device__ void operator()(uint32_t i, uint32_t ex, bool flagged, uint32_t) const {
    if (!flagged || ex >= cap) return;  // ex < cap always, by the count
    uint64_t k;
    (void)f.key_of(i, &k);
    ckey[ex] = k;
    cslot[ex] = i;
  }
};

// orand[0] |= every flagged key, orand[1] &= every flagged key
__global__ __launch_bounds__(256) void ftrl_state_bits_kernel(
    StateFlag f, uint32_t n, unsigned long long* __restrict__ orand) {
  uint64_t o = 0, a = ~0ull;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256u) {
    uint64_t k;
    if (f.key_of((uint32_t)i, &k) && k >= f.lo && k <= f.hi) {
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
}

// out[j] = the entry of the j-th key in key order: slot cslot[spos[j]]
__global__ __launch_bounds__(256) void ftrl_state_gather_kernel(
    FtrlTable T, uint32_t nslots, const uint64_t* __restrict__ skey,
    const uint32_t* __restrict__ spos, const uint32_t* __restrict__ cslot, uint32_t n,
    uint64_t* __restrict__ keys, uint64_t* __restrict__ pos, uint64_t* __restrict__ neg,
    double* __restrict__ w, double* __restrict__ z) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t at = spos[j];
  if (at >= n) return;  // never: a permutation of 0 .. n-1
  const uint32_t i = cslot[at];
  if (i > nslots) return;  // never
  const FtrlEntry* e = i < nslots ? &T.b[i / 3].e[i % 3] : &T.head->side;
  if (keys) keys[j] = skey[j];
  if (pos) pos[j] = e->pos;
  if (neg) neg[j] = e->neg;
  if (w) w[j] = e->w;
  if (z) z[j] = e->z;
}

constexpr uint32_t kStateGridCap = 2048;

// the blocks of launch_ftrl_state's work area for n entries
struct StateWork {
  size_t ckey, key_a, key_b, cslot, pos_a, pos_b, counts, dtotal, end;
  explicit StateWork(uint64_t n) {
    const size_t k8 = (size_t)(8 * n + 255) & ~(size_t)255, k4 = (size_t)(4 * n + 255) & ~(size_t)255;
    ckey = 0;
    key_a = ckey + k8;
    key_b = key_a + k8;
    cslot = key_b + k8;
    pos_a = cslot + k4;
    pos_b = pos_a + k4;
    counts = pos_b + k4;
    dtotal = counts + 4 * 256 * (size_t)blocks_of(n, kSortTile);
    end = dtotal + 4 * 256;
  }
};

}  // namespace

hipError_t launch_ftrl_import(const FtrlTable& T, const uint64_t* keys, const uint64_t* pos,
                              const uint64_t* neg, const double* w, const double* z, uint64_t n,
                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(&T.head->verdict, 0, 8, s);
  if (e != hipSuccess) return e;
  if (n > 1)
    hipLaunchKernelGGL(ftrl_check_kernel, dim3(blocks_of(n - 1, 256)), dim3(256), 0, s, keys, n,
                       T.head);
  hipLaunchKernelGGL(ftrl_import_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, T, keys, pos,
                     neg, w, z, n);
  return hipGetLastError();
}

size_t ftrl_state_count_words(const FtrlTable& T) {
  return blocks_of(3 * (T.mask + 1) + 1, kFlagTile);
}

int launch_ftrl_state_count(const FtrlTable& T, uint64_t lo, uint64_t hi, uint32_t* tile_sum,
                            unsigned long long* small, hipStream_t s) {
  const uint64_t nel = 3 * (T.mask + 1) + 1;
  if (nel > 0xffffffffull) return fail(PSG_ERR_SIZE, "FTRL state export: %llu slots >= 2^32",
                                        (unsigned long long)nel);
  const StateFlag f{T, lo, hi, (uint32_t)(nel - 1)};
  const unsigned long long init[3] = {0, ~0ull, 0};
  HIP_TRY(hipMemcpyAsync(small, init, sizeof init, hipMemcpyHostToDevice, s));
  const uint32_t nt = blocks_of(nel, kFlagTile);
  LAUNCH(flag_count_kernel<StateFlag>, nt, s, f, (uint32_t)nel, tile_sum);
  LAUNCH(row_scan_kernel, 1, s, tile_sum, nt, (uint32_t*)(small + 2));
  LAUNCH(ftrl_state_bits_kernel, std::min(blocks_of(nel, 256), kStateGridCap), s, f,
         (uint32_t)nel, small);
  return launched("ftrl state count");
}

size_t ftrl_state_work_bytes(uint64_t n) { return StateWork(n).end; }

int launch_ftrl_state(const FtrlTable& T, uint64_t lo, uint64_t hi, uint64_t n, uint64_t differ,
                      const uint32_t* tile_base, void* work, uint64_t* keys, uint64_t* pos,
                      uint64_t* neg, double* w, double* z, hipStream_t s) {
  if (n == 0) return PSG_OK;
  const uint64_t nel = 3 * (T.mask + 1) + 1;
  const StateWork W(n);
  char* base = (char*)work;
  uint64_t* ckey = (uint64_t*)(base + W.ckey);
  uint32_t* cslot = (uint32_t*)(base + W.cslot);
  const StateFlag f{T, lo, hi, (uint32_t)(nel - 1)};
  const StateEmit em{f, ckey, cslot, (uint32_t)n};
  LAUNCH((flag_emit_kernel<StateFlag, StateEmit>), blocks_of(nel, kFlagTile), s, f, em,
         (uint32_t)nel, tile_base);
  const SortBuffers sb{(uint64_t*)(base + W.key_a), (uint64_t*)(base + W.key_b),
                       (uint32_t*)(base + W.pos_a), (uint32_t*)(base + W.pos_b),
                       (uint32_t*)(base + W.counts), (uint32_t*)(base + W.dtotal)};
  const uint64_t* skey = nullptr;
  const uint32_t* spos = nullptr;
  if (int rc = enqueue_radix_sort(ckey, (uint32_t)n, differ, sb, &skey, &spos, s)) return rc;
  LAUNCH(ftrl_state_gather_kernel, blocks_of(n, 256), s, T, (uint32_t)(nel - 1), skey, spos,
         cslot, (uint32_t)n, keys, pos, neg, w, z);
  return launched("ftrl state export");
}

hipError_t launch_ftrl_push(const FtrlTable& T, const uint64_t* keys, const uint32_t* pos,
                            const uint32_t* neg, const double* grad, uint64_t n,
                            const FtrlParam& P, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(&T.head->verdict, 0, 8, s);
  if (e != hipSuccess) return e;
  if (n > 1)
    hipLaunchKernelGGL(ftrl_check_kernel, dim3(blocks_of(n - 1, 256)), dim3(256), 0, s, keys, n,
                       T.head);
  hipLaunchKernelGGL(ftrl_update_kernel, dim3(blocks_of(n, 256 * kFtrlIlp)), dim3(256), 0, s, T,
                     keys, pos, neg, grad, n, P);
  return hipGetLastError();
}

hipError_t launch_ftrl_pull(const FtrlTable& T, const uint64_t* keys, uint64_t n, double* out,
                            hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ftrl_pull_kernel, dim3(blocks_of(n, 256 * kFtrlIlp)), dim3(256), 0, s, T,
                     keys, n, out);
  return hipGetLastError();
}

hipError_t launch_ftrl_lookup(const FtrlTable& T, const uint64_t* keys, uint64_t n, uint64_t* pos,
                              uint64_t* neg, double* w, double* z, uint8_t* found,
                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ftrl_lookup_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, T, keys, n, pos,
                     neg, w, z, found);
  return hipGetLastError();
}

hipError_t launch_ftrl_rehash(const FtrlTable& from, const FtrlTable& to, hipStream_t s) {
  hipLaunchKernelGGL(ftrl_rehash_kernel, dim3(blocks_of(3 * (from.mask + 1), 256)), dim3(256), 0,
                     s, from, to);
  return hipGetLastError();
}

hipError_t launch_ftrl_count(const FtrlTable& T, hipStream_t s) {
  hipLaunchKernelGGL(ftrl_count_kernel, dim3(1), dim3(kFtrlSlots), 0, s, T.head);
  return hipGetLastError();
}

hipError_t launch_ftrl_norm(const FtrlTable& T, hipStream_t s) {
  const uint64_t nb = T.mask + 1;
  const uint64_t per = (nb + kFtrlPartials - 1) / kFtrlPartials;
  const uint32_t nparts = blocks_of(nb, per);
  hipLaunchKernelGGL(ftrl_count_kernel, dim3(1), dim3(kFtrlSlots), 0, s, T.head);
  hipLaunchKernelGGL(ftrl_norm_kernel, dim3(nparts), dim3(256), 0, s, T, per);
  hipLaunchKernelGGL(ftrl_norm_final_kernel, dim3(1), dim3(256), 0, s, T.head, nparts);
  return hipGetLastError();
}

hipError_t launch_ftrl_export(const FtrlTable& T, uint64_t* keys, double* w, uint64_t cap,
                              hipStream_t s) {
  hipError_t e = hipMemsetAsync(&T.head->res[4], 0, 8, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ftrl_export_kernel, dim3(blocks_of(3 * (T.mask + 1) + 1, 256)), dim3(256), 0,
                     s, T, keys, w, cap);
  return hipGetLastError();
}

}  // namespace psg
