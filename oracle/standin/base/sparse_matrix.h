// TEST INFRASTRUCTURE ONLY.  Stand-in for the reference's
// base/sparse_matrix.h (with the MatrixInfo message and the Matrix base of
// base/matrix.h), written for oracle/ref_localizer_shim.cc from what the
// reference's base/localizer.h calls: MatrixInfo's accessors, and
// SparseMatrix as a plain holder of info / offset / index / value.  Nothing
// is computed here (no times, no transpose).  It also brings in <thread>,
// which the reference's util/parallel_sort.h uses without including.  It
// holds no arithmetic or control flow of a pinned function.
#pragma once
#include <thread>

#include "base/range.h"
#include "base/shared_array.h"
#include "util/common.h"

namespace PS {
struct MatrixInfo {
  enum Type { DENSE = 1, SPARSE = 2, SPARSE_BINARY = 3 };
  Type type_ = SPARSE;
  bool row_major_ = true;
  uint32 sizeof_index_ = 0;
  uint64 nnz_ = 0;
  bool ins_info_ = true;
  PbRange row_, col_;

  Type type() const { return type_; }
  std::string DebugString() const { return std::string(); }
  bool row_major() const { return row_major_; }
  void set_sizeof_index(uint32 v) { sizeof_index_ = v; }
  void set_nnz(uint64 v) { nnz_ = v; }
  void clear_ins_info() { ins_info_ = false; }
  PbRange* mutable_row() { return &row_; }
  PbRange* mutable_col() { return &col_; }
};

template <typename V> class Matrix {
 public:
  virtual ~Matrix() {}
};
template <typename V> using MatrixPtr = std::shared_ptr<Matrix<V>>;

template <typename I, typename V> class SparseMatrix;
template <typename I, typename V>
using SparseMatrixPtr = std::shared_ptr<SparseMatrix<I, V>>;

template <typename I, typename V> class SparseMatrix : public Matrix<V> {
 public:
  SparseMatrix() {}
  SparseMatrix(const MatrixInfo& info, const SArray<size_t>& offset,
               const SArray<I>& index, const SArray<V>& value)
      : info_(info), offset_(offset), index_(index), value_(value) {}
  MatrixInfo info() const { return info_; }
  SArray<size_t> offset() const { return offset_; }
  SArray<I> index() const { return index_; }
  SArray<V> value() const { return value_; }

 private:
  MatrixInfo info_;
  SArray<size_t> offset_;
  SArray<I> index_;
  SArray<V> value_;
};
}  // namespace PS
