// psg_ftrl_find.h -- the read-only probes of the two resident FTRL tables
// (psg_internal.h's FtrlTable, psg_ftrl_rows.h's FtrlmTable), shared by the
// kernels that train them (psg_ftrl.hip, psg_ftrl_rows.hip) and the direct
// scorer (psg_score.hip).  Device code, file-local in each translation unit
// that includes this (anonymous namespace), as psg_sort.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psg_ftrl_rows.h"
#include "psg_internal.h"

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

// The row of `key` (!= 0), or kFtrlmNoRow, with the key's first slot s0 =
// idx[b] already read.  A slot whose row word is 0 was claimed by a key that
// found no row (an overflow, already counted): absent.
__device__ __forceinline__ uint64_t ftrlm_find_from(const FtrlmTable& T, uint64_t key, uint64_t b,
                                                    FtrlmSlot s) {
  for (uint64_t probe = 0; probe <= T.mask; ++probe) {
    if (s.key == key) return s.row != 0 && s.row < T.row_cap ? s.row : kFtrlmNoRow;
    if (s.key == 0) return kFtrlmNoRow;
    b = (b + 1) & T.mask;
    s = T.idx[b];
  }
  return kFtrlmNoRow;
}

// The row of `key`, or kFtrlmNoRow; key 0 has row 0 once it has been pushed.
__device__ __forceinline__ uint64_t ftrlm_find(const FtrlmTable& T, uint64_t key) {
  if (key == 0) return T.head->zero_present ? 0 : kFtrlmNoRow;
  const uint64_t b = fmix64(key) & T.mask;
  return ftrlm_find_from(T, key, b, T.idx[b]);
}

}  // namespace
}  // namespace psg
