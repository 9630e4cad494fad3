// psg_rows.h -- the shape arithmetic of the row-valued push kernels
// (psg_rows.hip): how a row of k values of V is dealt
// to lanes and how many server slots a tile holds.  One definition, read by
// the kernels, by the host code that sizes their launches and by
// psg_rows_shape() (include/psg.h), so a test that puts keys on a seam and
// the kernel agree on where the seam is.  Plain C++: no HIP call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PSG_ROWS_HD __host__ __device__
#else
#define PSG_ROWS_HD
#endif

namespace psg {
namespace rows {

constexpr int kMaxWidth = 256;       // k: values per key (psg_rows_max_width)
constexpr int kMaxTile = 1024;       // slots per tile, at most
constexpr int kAccBytes = 64 * 1024; // a tile's accumulators acc[T][k], at most
// LDS of one workgroup: accumulators, the tile's keys (8 B per slot), the
// contributor counts (4 B per slot) and kLdsFixed bytes of bookkeeping (the
// table of the 64 pushes being folded).  Two workgroups share a CU's 160 KB.
constexpr int kLdsFixed = 2048;
constexpr int kLdsBudget = 80 * 1024;
// the fold kernel's one static allocation: the largest lds_bytes()
constexpr int kLdsAlloc = kAccBytes + kMaxTile * 12 + kLdsFixed;
constexpr int kThreads = 256;        // one workgroup: 4 waves
constexpr int kUnitBytes = 16;       // one lane access
constexpr int kItemRows = 4;         // rows a lane group holds in flight per step

struct Shape {
  int T;  // slots per tile (a power of two)
  int L;  // lanes per row (a power of two, <= 64)
  int E;  // elements per lane access (16 B / sizeof(V))
  int R;  // rows a wave handles per pass (64 / L)
};

PSG_ROWS_HD constexpr bool valid(int vbytes, int k) {
  return (vbytes == 4 || vbytes == 8) && k >= 1 && k <= kMaxWidth;
}

// T: the largest power of two <= kMaxTile whose accumulators fit kAccBytes.
// L: the smallest power of two of lanes whose accesses cover the row, 64 at
// most; a row wider than 64 E elements takes loops(s, k) > 1 accesses per lane.
PSG_ROWS_HD constexpr Shape shape_of(int vbytes, int k) {
  Shape s{kMaxTile, 1, kUnitBytes / vbytes, 64};
  while (s.T * k * vbytes > kAccBytes) s.T >>= 1;
  while (s.L < 64 && s.L * s.E < k) s.L <<= 1;
  s.R = 64 / s.L;
  return s;
}
PSG_ROWS_HD constexpr int loops(const Shape& s, int k) { return (k + s.L * s.E - 1) / (s.L * s.E); }
constexpr int kMaxLoops = 2;  // f64, k > 128

PSG_ROWS_HD constexpr size_t lds_bytes(int vbytes, int k) {
  const Shape s = shape_of(vbytes, k);
  return (size_t)s.T * k * vbytes + (size_t)s.T * 12 + kLdsFixed;
}

// the floor of T, and the budget, at the widest rows
static_assert(shape_of(8, kMaxWidth).T == 32 && shape_of(4, kMaxWidth).T == 64, "smallest tiles");
static_assert(shape_of(4, 1).T == kMaxTile && shape_of(8, 8).T == kMaxTile, "largest tiles");
static_assert(kLdsAlloc <= kLdsBudget && lds_bytes(4, 16) == (size_t)kLdsAlloc, "the allocation");
static_assert(lds_bytes(4, kMaxWidth) <= kLdsBudget && lds_bytes(8, kMaxWidth) <= kLdsBudget &&
                  lds_bytes(4, 16) <= kLdsBudget && lds_bytes(8, 8) <= kLdsBudget,
              "two workgroups per CU");
static_assert(loops(shape_of(8, kMaxWidth), kMaxWidth) == kMaxLoops &&
                  loops(shape_of(4, kMaxWidth), kMaxWidth) == 1,
              "accesses per lane and row");

}  // namespace rows
}  // namespace psg
