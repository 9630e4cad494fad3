// TEST INFRASTRUCTURE ONLY.  C entry points onto the reference's own
// LM::FTRLModel<uint64, double> (reference src/linear_method/ftrl_model.h
// with src/base/soft_thresholding.h), compiled in place from the reference
// tree by oracle/Makefile into oracle/_ref/.  oracle/standin/ supplies the
// containers, message structs, config structs and CHECK macros the header
// asks for.  Used by tools/record_reference.py and
// tests/test_reference_pin.py to pin tests/ftrl_ref.py's restatements.
//
// PINNED here: setLearningRate, setPenalty, setValue, getValue, nnz, objv,
// writeToFile.  OURS: the entry lookup below (a find on model_, which is
// protected, hence the derived class) and the packing of a message.
#include "linear_method/ftrl_model.h"

using namespace PS;

namespace {
struct Model : LM::FTRLModel<uint64, double> {
  size_t entries() const { return model_.size(); }
  bool entry(uint64 k, uint64* p, uint64* n, double* w, double* z) const {
    auto it = model_.find(k);
    if (it == model_.end()) return false;
    *p = it->second.pos; *n = it->second.neg;
    *w = it->second.w; *z = it->second.z;
    return true;
  }
};

template <typename T> SArray<T> copy_in(const T* p, size_t n) {
  SArray<T> a(n);
  if (n) memcpy(a.data(), p, n * sizeof(T));
  return a;
}
}  // namespace

extern "C" {

void* ref_ftrl_create(double alpha, double beta, double lambda1,
                      double lambda2) {
  Model* m = new Model();
  LearningRateConfig lr;
  lr.a = alpha; lr.b = beta;
  m->setLearningRate(lr);
  PenaltyConfig pc;
  pc.l = {lambda1, lambda2};
  m->setPenalty(pc);
  return m;
}
void ref_ftrl_destroy(void* h) { delete (Model*)h; }

void ref_ftrl_set_value(void* h, const uint64* keys, const uint32* pos,
                        const uint32* neg, const double* grad, size_t n) {
  MessagePtr msg(new Message());
  msg->key = SArray<char>(copy_in(keys, n));
  msg->addValue(copy_in(pos, n));
  msg->addValue(copy_in(neg, n));
  msg->addValue(copy_in(grad, n));
  ((Model*)h)->setValue(msg);
}

// inserts a zero entry for every absent key, as the reference's pull does
void ref_ftrl_get_value(void* h, const uint64* keys, size_t n, double* out) {
  MessagePtr msg(new Message());
  msg->key = SArray<char>(copy_in(keys, n));
  ((Model*)h)->getValue(msg);
  SArray<double> val(msg->value.back());
  if (n) memcpy(out, val.data(), n * sizeof(double));
}

size_t ref_ftrl_nnz(void* h) { return ((Model*)h)->nnz(); }
double ref_ftrl_objv(void* h) { return ((Model*)h)->objv(); }
size_t ref_ftrl_entries(void* h) { return ((Model*)h)->entries(); }

void ref_ftrl_write_to_file(void* h, const char* path) {
  DataConfig dc;
  dc.f = {path};
  ((Model*)h)->writeToFile(dc);
}

void ref_ftrl_lookup(void* h, const uint64* keys, size_t n, uint64* pos,
                     uint64* neg, double* w, double* z, unsigned char* found) {
  for (size_t i = 0; i < n; ++i) {
    pos[i] = neg[i] = 0;
    w[i] = z[i] = 0;
    found[i] = ((Model*)h)->entry(keys[i], pos + i, neg + i, w + i, z + i);
  }
}

}  // extern "C"
