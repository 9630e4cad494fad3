// TEST INFRASTRUCTURE ONLY.  Stand-in for the reference's SArray (a shared,
// reinterpretable, sliceable array), written for oracle/ref_*_shim.cc from
// what the pinned code calls on it.  Every member here is OURS and therefore
// not pinned by the shims (findRange is pinned separately by the reference's
// shared_array_test vectors).  It holds no arithmetic or control flow of a
// pinned function.
#pragma once
#include "base/range.h"
#include "util/common.h"

namespace PS {
template <typename V> class SArray {
 public:
  SArray() {}
  explicit SArray(size_t n)
      : p_(new std::vector<char>(n * sizeof(V))), off_(0), n_(n) {}
  SArray(size_t n, V fill)
      : p_(new std::vector<char>(n * sizeof(V))), off_(0), n_(n) {
    std::fill(begin(), end(), fill);
  }
  // the same bytes seen as another element type
  template <typename W> explicit SArray(const SArray<W>& o)
      : p_(o.p_), off_(o.off_), n_(o.n_ * sizeof(W) / sizeof(V)) {}
  template <typename W> void operator=(const SArray<W>& o) {
    p_ = o.p_; off_ = o.off_; n_ = o.n_ * sizeof(W) / sizeof(V);
  }

  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  V* data() const { return p_ ? (V*)(p_->data() + off_) : nullptr; }
  V* begin() const { return data(); }
  V* end() const { return data() + n_; }
  V& operator[](size_t i) const { return data()[i]; }
  V& back() const { return data()[n_ - 1]; }

  void clear() { p_.reset(); off_ = 0; n_ = 0; }
  void resize(size_t n) {
    std::shared_ptr<std::vector<char>> q(new std::vector<char>(n * sizeof(V)));
    if (n_ && n) memcpy(q->data(), data(), std::min(n, n_) * sizeof(V));
    p_ = q; off_ = 0; n_ = n;
  }
  void setZero() { if (n_) memset(data(), 0, n_ * sizeof(V)); }
  void pushBack(const V& x) {
    if (!p_ || off_) resize(n_);
    p_->resize((n_ + 1) * sizeof(V));
    data()[n_++] = x;
  }

  SArray segment(const SizeR& r) const {
    SArray s;
    s.p_ = p_; s.off_ = off_ + r.begin() * sizeof(V); s.n_ = r.size();
    return s;
  }
  // [lower_bound(r.begin), lower_bound(r.end)) over sorted contents
  SizeR findRange(const Range<V>& r) const {
    return SizeR(std::lower_bound(begin(), end(), r.begin()) - begin(),
                 std::lower_bound(begin(), end(), r.end()) - begin());
  }

  std::shared_ptr<std::vector<char>> p_;
  size_t off_ = 0, n_ = 0;
};
template <typename V> using SArrayList = std::vector<SArray<V>>;
}  // namespace PS
