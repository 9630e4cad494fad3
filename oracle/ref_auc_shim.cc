// TEST INFRASTRUCTURE ONLY.  C entry points onto the reference's own AUC
// (reference src/base/auc.h) and Evaluation<double> (src/base/evaluation.h),
// compiled in place from the reference tree by oracle/Makefile into
// oracle/_ref/.  oracle/standin/ supplies SArray, the AUCData message
// (proto/evaluation.pb.h) and the CHECK macros.  Used by
// tools/record_reference.py and tests/test_reference_pin.py to pin
// tests/auc_ref.py's restatements.
//
// PINNED here: setGoodness, compute<double>, merge, accuracy, evaluate and
// Evaluation<double>::auc (with the std::sort it calls).  OURS: packing the
// flat arrays into SArray / AUCData and back, and reading the root's two maps
// (they are private, so the header is included with private opened; nothing
// of it is re-implemented).
#include <thread>  // util/parallel_sort.h names std::thread without it

#include "base/shared_array.h"
#include "proto/evaluation.pb.h"
#define private public
#include "base/auc.h"
#undef private
#include "base/evaluation.h"

using namespace PS;

namespace {
SArray<double> copy_in(const double* p, size_t n) {
  SArray<double> a(n);
  if (n) memcpy(a.data(), p, n * sizeof(double));
  return a;
}
template <typename K, typename C>
void copy_out(const std::vector<K>& k, const std::vector<C>& c, K* ko, C* co) {
  if (k.size()) memcpy(ko, k.data(), k.size() * sizeof(K));
  if (c.size()) memcpy(co, c.data(), c.size() * sizeof(C));
}
void map_out(const std::map<int64, uint64>& m, int64* k, uint64* c) {
  size_t i = 0;
  for (auto& it : m) { k[i] = it.first; c[i] = it.second; ++i; }
}
}  // namespace

extern "C" {

// compute<double> of n >= 1 examples; every output holds up to n entries
void ref_auc_compute(int64 goodness, const double* label, const double* predict,
                     size_t n, int64* tp_key, uint64* tp_count, size_t* ntp,
                     int64* fp_key, uint64* fp_count, size_t* nfp) {
  AUC auc;
  auc.setGoodness(goodness);
  AUCData res;
  auc.compute(copy_in(label, n), copy_in(predict, n), &res);
  *ntp = res.tp_key_.size();
  *nfp = res.fp_key_.size();
  copy_out(res.tp_key_, res.tp_count_, tp_key, tp_count);
  copy_out(res.fp_key_, res.fp_count_, fp_key, fp_count);
}

// the root: merge any number of AUCData, then accuracy / evaluate
void* ref_auc_create(int64 goodness) {
  AUC* a = new AUC();
  a->setGoodness(goodness);
  return a;
}
void ref_auc_destroy(void* h) { delete (AUC*)h; }

void ref_auc_merge(void* h, const int64* tp_key, const uint64* tp_count,
                   size_t ntp, const int64* fp_key, const uint64* fp_count,
                   size_t nfp) {
  AUCData d;
  d.tp_key_.assign(tp_key, tp_key + ntp);
  d.tp_count_.assign(tp_count, tp_count + ntp);
  d.fp_key_.assign(fp_key, fp_key + nfp);
  d.fp_count_.assign(fp_count, fp_count + nfp);
  ((AUC*)h)->merge(d);
}

double ref_auc_accuracy(void* h, double threshold) {
  return ((AUC*)h)->accuracy(threshold);
}
double ref_auc_evaluate(void* h) { return ((AUC*)h)->evaluate(); }

// the two maps in their own order (NULL outputs only report the sizes)
void ref_auc_maps(void* h, size_t* ntp, size_t* nfp, int64* tp_key,
                  uint64* tp_count, int64* fp_key, uint64* fp_count) {
  AUC* a = (AUC*)h;
  *ntp = a->tp_count_.size();
  *nfp = a->fp_count_.size();
  if (tp_key) map_out(a->tp_count_, tp_key, tp_count);
  if (fp_key) map_out(a->fp_count_, fp_key, fp_count);
}

double ref_eval_auc(const double* label, const double* predict, size_t n) {
  return Evaluation<double>::auc(copy_in(label, n), copy_in(predict, n));
}

}  // extern "C"
