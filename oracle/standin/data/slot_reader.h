// TEST INFRASTRUCTURE ONLY.  Stand-in for the reference's data/slot_reader.h,
// written for oracle/ref_localizer_shim.cc: the members that
// Localizer::remapIndex(int, const SArray<I>&, SlotReader*) names, declared
// only.  That overload is never instantiated, so none of them is defined.
// It holds no arithmetic or control flow of a pinned function.
#pragma once
#include "base/shared_array.h"
#include "base/sparse_matrix.h"

namespace PS {
class SlotReader {
 public:
  template <typename V> MatrixInfo info(int slot_id) const;
  template <typename V> SArray<V> value(int slot_id) const;
  SArray<uint64> index(int slot_id);
  SArray<size_t> offset(int slot_id);
};
}  // namespace PS
