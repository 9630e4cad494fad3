// psg_colsum.cc -- psg_sum_blocked_host (include/psg.h): the blocked
// summation order B of psg_colsum.hip restated on the host, one IEEE add per
// `+` (built with -ffp-contract=off; there is no multiply to contract).
// Host code only, and nothing of the library's but the header.
#include <new>
#include <vector>

#include "../../include/psg.h"
#include "psg_colsum.h"

namespace {

using psg::kColLanes;
using psg::kColSeg;
using psg::kColSerial;

// B of n <= kColSeg terms, `stride` doubles apart
double block_sum(const double* t, size_t n, size_t stride) {
  if (n <= kColSerial) {
    double a = 0.0;
    for (size_t i = 0; i < n; ++i) a = a + t[i * stride];
    return a;
  }
  double p[kColLanes];
  for (size_t j = 0; j < kColLanes; ++j) {
    double a = 0.0;
    for (size_t i = j; i < n; i += kColLanes) a = a + t[i * stride];
    p[j] = a;
  }
  for (size_t d = kColLanes / 2; d >= 1; d >>= 1)
    for (size_t j = 0; j < d; ++j) p[j] = p[j] + p[j + d];
  return p[0];
}

}  // namespace

extern "C" int psg_sum_blocked_host(const double* t, size_t n, size_t stride, double* out) {
  if (!out || (n && !t) || (n > 1 && stride == 0)) return PSG_ERR_ARG;
  if (n <= kColSeg) {
    *out = block_sum(t, n, stride);
    return PSG_OK;
  }
  std::vector<double> q;
  try {
    q.resize((n + kColSeg - 1) / kColSeg);
  } catch (const std::bad_alloc&) {
    return PSG_ERR_OOM;
  }
  for (size_t k = 0; k < q.size(); ++k) {
    const size_t at = k * kColSeg, len = n - at < kColSeg ? n - at : kColSeg;
    q[k] = block_sum(t + at * stride, len, stride);
  }
  size_t m = q.size();  // the next levels in place: q[k] is read before it is written
  while (m > kColSeg) {
    const size_t segs = (m + kColSeg - 1) / kColSeg;
    for (size_t k = 0; k < segs; ++k) {
      const size_t at = k * kColSeg, len = m - at < kColSeg ? m - at : kColSeg;
      q[k] = block_sum(q.data() + at, len, 1);
    }
    m = segs;
  }
  *out = block_sum(q.data(), m, 1);
  return PSG_OK;
}
