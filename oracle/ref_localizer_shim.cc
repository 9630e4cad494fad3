// TEST INFRASTRUCTURE ONLY.  C entry points onto the reference's own
// Localizer<uint64, double> (reference src/base/localizer.h, with the
// parallelSort of src/util/parallel_sort.h under it), compiled in place from
// the reference tree by oracle/Makefile into oracle/_ref/.  oracle/standin/
// supplies SArray, MatrixInfo / SparseMatrix as plain holders
// (base/sparse_matrix.h), SlotReader's declarations and the CHECK macros.
// Used by tools/record_reference.py and tests/test_reference_pin.py to pin
// tests/worker_ref.py's localizer restatements.
//
// PINNED here: countUniqIndex(idx, uniq_idx, idx_frq) and
// remapIndex(info, offset, index, value, idx_dict), with parallelSort,
// std::sort and std::inplace_merge below them.  OURS: packing the flat arrays
// into SArray and back, and taking the returned SparseMatrix apart.
#include "util/common.h"

int FLAGS_num_threads = 1;

#include "base/localizer.h"  // last: its #pragma pack(4) is never popped

using namespace PS;

namespace {
typedef Localizer<uint64, double> Loc;

template <typename T, typename S> SArray<T> copy_in(const S* p, size_t n) {
  SArray<T> a(n);
  for (size_t i = 0; i < n; ++i) a[i] = (T)p[i];
  return a;
}
}  // namespace

extern "C" {

void* ref_loc_create() { return new Loc(); }
void ref_loc_destroy(void* h) { delete (Loc*)h; }

// countUniqIndex of n >= 1 ids; uniq / frq hold up to n entries.  Returns the
// number of unique ids.  The localizer keeps its sorted pairs for remap.
size_t ref_loc_count_uniq(void* h, const uint64* idx, size_t n, int threads,
                          uint64* uniq, uint32* frq) {
  FLAGS_num_threads = threads;
  SArray<uint64> u;
  SArray<uint32> f;
  ((Loc*)h)->countUniqIndex(copy_in<uint64>(idx, n), &u, &f);
  for (size_t i = 0; i < u.size(); ++i) uniq[i] = u[i];
  for (size_t i = 0; i < f.size(); ++i) frq[i] = f[i];
  return u.size();
}

// remapIndex after ref_loc_count_uniq of the same index.  value == NULL: a
// binary matrix.  Returns 0 and fills the outputs (new_offset: noffset
// entries, new_index / new_value: up to n), or -1 when the reference returns
// a null pointer.
int ref_loc_remap(void* h, const uint64* offset, size_t noffset,
                  const uint64* index, size_t n, const double* value,
                  const uint64* dict, size_t ndict, int threads,
                  uint64* new_offset, uint32* new_index, size_t* nindex,
                  double* new_value, size_t* nvalue) {
  FLAGS_num_threads = threads;
  MatrixInfo info;
  MatrixPtr<double> m = ((Loc*)h)->remapIndex(
      info, copy_in<size_t>(offset, noffset), copy_in<uint64>(index, n),
      value ? copy_in<double>(value, n) : SArray<double>(),
      copy_in<uint64>(dict, ndict));
  if (!m) return -1;
  auto sm = std::static_pointer_cast<SparseMatrix<uint32, double>>(m);
  SArray<size_t> no = sm->offset();
  SArray<uint32> ni = sm->index();
  SArray<double> nv = sm->value();
  for (size_t i = 0; i < no.size(); ++i) new_offset[i] = no[i];
  *nindex = ni.size();
  if (ni.size()) memcpy(new_index, ni.data(), ni.size() * sizeof(uint32));
  *nvalue = nv.size();
  if (nv.size()) memcpy(new_value, nv.data(), nv.size() * sizeof(double));
  return 0;
}

}  // extern "C"
