// ftrl_model.h -- host C++ mirror of PS::LM::FTRLModel<Key, V> over the psg
// C ABI.
//
// Reference: wakensky/parameter_server src/linear_method/ftrl_model.h:12-69
// (the class), :72-78 (getValue), :80-112 (setValue), :24-29 (writeToFile),
// :31-32 (objv, nnz); driven by src/linear_method/ftrl.cc.  The method names
// and argument meaning are the reference's; the map behind them is a hash
// table resident in the HBM of one MI355X and every operation is a libpsg
// call (include/psg.h, which lists the defined deviations: a pull does not
// insert, the norms are a reduction, a message must be strictly increasing,
// the dump is sorted by key).  Header-only, plain C++11 + the C ABI, like
// kv_vector.h, whose Message / Error / check it shares.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <istream>
#include <map>
#include <numeric>

#include "kv_vector.h"

namespace psg {

template <typename V>
class FTRLModel {
  static_assert(sizeof(V) == sizeof(double) && DType<V>::value == PSG_F64,
                "the FTRL model is double (ftrl.h:26)");

 public:
  explicit FTRLModel(int device = 0, size_t capacity_hint = 0) : hint_(capacity_hint) {
    psg_ctx* c = nullptr;
    check(psg_create(device, PSG_F64, 0, &c));
    ctx_.reset(c, [](psg_ctx* p) { psg_destroy(p); });
  }

  // LearningRateConfig alpha / beta and PenaltyConfig lambda(0) / lambda(1)
  // (ftrl_model.h:15-22), set before the first message as FTRL::init does
  void setLearningRate(V alpha, V beta) {
    fresh("setLearningRate");
    p_.alpha = alpha;
    p_.beta = beta;
  }
  void setPenalty(V lambda1, V lambda2) {
    fresh("setPenalty");
    p_.lambda1 = lambda1;
    p_.lambda2 = lambda2;
  }
  // room for this many keys: pushes then allocate nothing
  void reserve(size_t entries) { check(psg_ftrl_reserve(model(), entries)); }

  // setValue (ftrl_model.h:80-112): value = {uint32 pos, uint32 neg, V grad}
  void setValue(const MessagePtr& msg) {
    const size_t n = msg->key.size();
    if (msg->value.size() != 3) throw Error(PSG_ERR_SIZE, "FTRL needs 3 value arrays");  // :85
    if (msg->value[0].size() != n * sizeof(uint32_t) ||
        msg->value[1].size() != n * sizeof(uint32_t) || msg->value[2].size() != n * sizeof(V))
      throw Error(PSG_ERR_SIZE, "value array size != key count");  // :86-88
    if (n == 0) return;
    check(psg_ftrl_push(model(), msg->key.data(), n, (const uint32_t*)msg->value[0].data(),
                        (const uint32_t*)msg->value[1].data(),
                        (const double*)msg->value[2].data()));
  }

  // getValue (ftrl_model.h:72-78): the reply's one value array
  void getValue(const MessagePtr& msg) {
    std::vector<V> out(msg->key.size());
    if (!out.empty()) check(psg_ftrl_pull(model(), msg->key.data(), out.size(), out.data()));
    msg->addValue(out);
  }

  V objv() {  // :31
    double n1 = 0, n2 = 0;
    check(psg_ftrl_status(model(), nullptr, nullptr, &n1, &n2));
    return n1 * p_.lambda1 + .5 * p_.lambda2 * std::sqrt(n2);
  }
  size_t nnz() {  // :32
    size_t z = 0;
    check(psg_ftrl_status(model(), nullptr, &z, nullptr, nullptr));
    return z;
  }

  // writeToFile (:24-29): "key \t w" per nonzero weight, here sorted by key
  void writeToFile(const std::string& path) {
    size_t n = 0;
    int rc = psg_ftrl_export(model(), nullptr, nullptr, 0, &n);
    if (rc != PSG_ERR_SIZE) check(rc);
    std::vector<Key> k(n);
    std::vector<V> w(n);
    if (n) check(psg_ftrl_export(model(), k.data(), w.data(), n, &n));
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return k[a] < k[b]; });
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) throw Error(PSG_ERR_ARG, "cannot open " + path);  // CHECK(out.good())
    for (size_t i : order)
      std::fprintf(f, "%llu\t%g\n", (unsigned long long)k[i], (double)w[i]);
    std::fclose(f);
  }

  // The hooks the reference leaves empty (ftrl_model.h:41-44).  A model's
  // whole entries, sorted by key.
  struct State {
    std::vector<Key> key;
    std::vector<uint64_t> pos, neg;
    std::vector<V> w, z;
  };
  // getReplica: every entry with first <= key <= last (psg_ftrl_export_state)
  State exportState(Key first = 0, Key last = ~(Key)0) {
    const uint64_t range[2] = {first, last};
    size_t n = 0;
    int rc = psg_ftrl_export_state(model(), range, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   0, &n);
    if (rc != PSG_ERR_SIZE) check(rc);
    State s;
    s.key.resize(n);
    s.pos.resize(n);
    s.neg.resize(n);
    s.w.resize(n);
    s.z.resize(n);
    if (n)
      check(psg_ftrl_export_state(model(), range, s.key.data(), s.pos.data(), s.neg.data(),
                                  s.w.data(), s.z.data(), n, &n));
    return s;
  }
  // recoverFrom / setReplica: an upsert of whole entries, strictly increasing
  // by key (psg_ftrl_import)
  void importState(const State& s) {
    const size_t n = s.key.size();
    if (s.pos.size() != n || s.neg.size() != n || s.w.size() != n || s.z.size() != n)
      throw Error(PSG_ERR_SIZE, "state array size != key count");
    check(psg_ftrl_import(model(), s.key.data(), n, s.pos.data(), s.neg.data(), s.w.data(),
                          s.z.data()));
  }

  // The parse of ModelEvaluation::run (model_evaluation.h:16-27): "key value"
  // pairs as `in >> k >> v`, a later pair overriding an earlier one.  Unlike
  // the reference's loop it does not assign weight[0] from the failed
  // extraction after the last line; a trailing unpaired token is an error.
  // Real: the type a weight is rounded through (the reference's is float).
  template <typename Real = V>
  static std::map<Key, V> parseModel(std::istream& in) {
    std::map<Key, V> weight;
    Key k;
    while (in >> k) {
      Real v;
      if (!(in >> v)) throw Error(PSG_ERR_ARG, "model file: a key without a value");
      weight[k] = (V)v;
    }
    if (!in.eof()) throw Error(PSG_ERR_ARG, "model file: a key that is no uint64");
    return weight;
  }
  // ... and the load: the weights-only import.  The model is evaluation-only
  // afterwards (psg_ftrl_frozen): pulls work, pushes are PSG_ERR_ARG.
  template <typename Real = V>
  void readFromFile(const std::string& path) {
    std::ifstream in(path);
    if (!in.good()) throw Error(PSG_ERR_ARG, "cannot open " + path);
    const std::map<Key, V> weight = parseModel<Real>(in);
    std::vector<Key> k;
    std::vector<V> w;
    for (const auto& kv : weight) {
      k.push_back(kv.first);
      w.push_back(kv.second);
    }
    if (w.empty()) w.reserve(1);  // a non-null pointer: an empty file still freezes
    check(psg_ftrl_import(model(), k.data(), k.size(), nullptr, nullptr, w.data(), nullptr));
  }
  bool frozen() {
    int f = 0;
    check(psg_ftrl_frozen(model(), &f));
    return f != 0;
  }

 private:
  void fresh(const char* what) {
    if (live_) throw Error(PSG_ERR_ARG, std::string(what) + " after the model's first message");
  }
  psg_ctx* model() {
    if (!live_) {
      check(psg_ftrl_init(ctx_.get(), &p_, hint_));
      live_ = true;
    }
    return ctx_.get();
  }

  std::shared_ptr<psg_ctx> ctx_;
  psg_ftrl_param p_ = {1, 1, 0, 0};
  size_t hint_ = 0;
  bool live_ = false;
};

}  // namespace psg
