// psg_auc_dev.h -- what psg_auc.hip (one histogram) and psg_auc_rows.hip (m
// histograms in one table) share on the device: the key of a prediction, the
// wave's fold of a batch's smallest and largest key, and the digit mask of a
// span.  File-local in each translation unit that includes this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psg {
namespace {

constexpr uint64_t kSignBit = 1ull << 63;
constexpr uint32_t kGridCap = 2048;  // workgroups of a grid-stride launch

// auc.h:75 on x86-64: a NaN product or one of magnitude >= 2^63 converts to
// INT64_MIN there (the device's own conversion saturates)
__device__ __forceinline__ uint64_t biased_key(double predict, double goodness) {
  const double p = predict * goodness;
  const long long k = fabs(p) < 9223372036854775808.0 ? (long long)p : (long long)kSignBit;
  return (uint64_t)k ^ kSignBit;
}

__device__ __forceinline__ void fold_min_max(uint64_t lo, uint64_t hi,
                                             unsigned long long* __restrict__ minmax) {
  for (int s = 32; s >= 1; s >>= 1) {
    const uint64_t a = __shfl_xor(lo, s, 64), b = __shfl_xor(hi, s, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicMin(minmax, (unsigned long long)lo);
    atomicMax(minmax + 1, (unsigned long long)hi);
  }
}

// every bit up to the highest one of `span`: the digits two keys within that
// span of each other can differ in (after the smallest is subtracted)
inline uint64_t bits_up_to(uint64_t span) {
  uint64_t b = 0;
  while (b < span) b = (b << 1) | 1u;
  return b;
}

}  // namespace
}  // namespace psg
