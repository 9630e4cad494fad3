// C++ driver for the checkpoint side of the FTRLModel adapter
// (parameter_server_amd/csrc/ftrl_model.h): exportState / importState /
// readFromFile, built with plain g++ against libpsg.so.
//
//   test_ftrl_checkpoint host MODEL EXPECT [f32]  -- the parse only (no GPU)
//   test_ftrl_checkpoint gpu MODEL EXPECT [f32]   -- and the models on device 0
//
// MODEL is a "key value" model file as ModelEvaluation::run reads them;
// EXPECT is what the Python side says the map must be: a count, then one
// "key weight-bits(hex)" line per key in key order.  f32: the weights are
// rounded through float (the reference's Real).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "../../parameter_server_amd/csrc/ftrl_model.h"

using psg::Key;
using psg::Message;
using psg::MessagePtr;
typedef psg::FTRLModel<double> Model;

static int failures = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: EXPECT(%s)\n", __FILE__, __LINE__, #c); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static uint64_t to_bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

static bool read_expect(const char* path, std::map<Key, uint64_t>* m) {
  std::ifstream in(path);
  size_t n;
  if (!(in >> n)) return false;
  for (size_t i = 0; i < n; ++i) {
    Key k;
    uint64_t b;
    if (!(in >> std::dec >> k >> std::hex >> b)) return false;
    (*m)[k] = b;
  }
  return m->size() == n;
}

static std::map<Key, double> parse(const char* path, bool f32) {
  std::ifstream in(path);
  return f32 ? Model::parseModel<float>(in) : Model::parseModel<double>(in);
}

static bool parse_throws(const std::string& text) {
  std::istringstream in(text);
  try {
    Model::parseModel<double>(in);
  } catch (const psg::Error& e) {
    return e.status() == PSG_ERR_ARG;
  }
  return false;
}

static void host_tests(const char* model, const std::map<Key, uint64_t>& want, bool f32) {
  const std::map<Key, double> got = parse(model, f32);
  EXPECT(got.size() == want.size());
  size_t bad = 0;
  for (const auto& kv : got) {
    auto it = want.find(kv.first);
    bad += it == want.end() || it->second != to_bits(kv.second);
  }
  EXPECT(bad == 0);
  EXPECT(parse_throws("1\t2\n3\n"));   // a key without a value
  EXPECT(parse_throws("1\t2\nx\t3\n"));
  std::istringstream empty("\n \n");
  EXPECT(Model::parseModel<double>(empty).empty());  // no phantom key 0
}

// n strictly increasing keys from a small generator, with their message;
// the keys are dense enough that two messages overlap
static MessagePtr message(uint64_t seed, size_t n) {
  MessagePtr m(new Message());
  std::vector<uint32_t> pos(n), neg(n);
  std::vector<double> grad(n);
  uint64_t x = seed, key = 0;
  for (size_t i = 0; i < n; ++i) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    key += 1 + (x >> 40) % 7;
    m->key.push_back(key * 1000003ull);
    pos[i] = (uint32_t)(x >> 20) % 6;
    neg[i] = (uint32_t)(x >> 30) % 6;
    grad[i] = ((double)(x >> 11) / 9007199254740992.0 - 0.5) * 6;
  }
  m->addValue(pos);
  m->addValue(neg);
  m->addValue(grad);
  return m;
}

static std::vector<double> pull(Model& model, const std::vector<Key>& keys) {
  MessagePtr req(new Message());
  req->key = keys;
  model.getValue(req);
  return req->valueAs<double>(0);
}

static void gpu_tests(const char* model_path, const std::map<Key, uint64_t>& want, bool f32) {
  Model a(0, 64);
  a.setLearningRate(1, 1);
  a.setPenalty(1, 0.1);
  const MessagePtr m1 = message(1, 700), m2 = message(2, 700), m3 = message(1, 500);
  a.setValue(m1);
  a.setValue(m2);

  // exportState -> importState into a second model: identical from then on
  const Model::State st = a.exportState();
  EXPECT(!st.key.empty() && st.key.size() == st.z.size());
  for (size_t i = 1; i < st.key.size(); ++i) EXPECT(st.key[i - 1] < st.key[i]);
  Model b(0, 64);
  b.setLearningRate(1, 1);
  b.setPenalty(1, 0.1);
  b.importState(st);
  EXPECT(!b.frozen());
  a.setValue(m3);
  b.setValue(m3);
  std::vector<Key> keys = m1->key;
  keys.insert(keys.end(), m2->key.begin(), m2->key.end());
  keys.push_back(12345);  // never pushed
  const std::vector<double> wa = pull(a, keys), wb = pull(b, keys);
  size_t bad = 0, nonzero = 0;
  for (size_t i = 0; i < wa.size(); ++i) {
    bad += to_bits(wa[i]) != to_bits(wb[i]);
    nonzero += wa[i] != 0;
  }
  EXPECT(bad == 0 && nonzero > 100);
  EXPECT(a.nnz() == b.nnz() && a.nnz() > 0);
  // a range of the image is that part of it
  const Key mid = st.key[st.key.size() / 2];
  const Model::State lo = b.exportState(0, mid), hi = b.exportState(mid + 1);
  EXPECT(lo.key.size() + hi.key.size() == b.exportState().key.size());
  EXPECT(lo.key.back() == mid);
  // an image that is not strictly increasing is refused
  bool threw = false;
  try {
    Model::State s2 = st;
    s2.key[1] = s2.key[0];
    b.importState(s2);
    (void)b.nnz();  // the next synchronising call reports it
  } catch (const psg::Error& e) {
    threw = e.status() == PSG_ERR_UNSORTED;
  }
  EXPECT(threw);
  EXPECT(a.nnz() == b.nnz());

  // readFromFile: a frozen model whose pulls are the file's map
  Model c(0, 64);
  if (f32) {
    c.readFromFile<float>(model_path);
  } else {
    c.readFromFile(model_path);
  }
  EXPECT(c.frozen());
  std::vector<Key> wk;
  for (const auto& kv : want) wk.push_back(kv.first);
  const std::vector<double> wc = pull(c, wk);
  bad = 0;
  for (size_t i = 0; i < wk.size(); ++i) bad += to_bits(wc[i]) != want.at(wk[i]);
  EXPECT(bad == 0 && !wk.empty());
  threw = false;
  try {
    c.setValue(m1);
  } catch (const psg::Error& e) {
    threw = e.status() == PSG_ERR_ARG;
  }
  EXPECT(threw);
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s host|gpu MODEL EXPECT [f32]\n", argv[0]);
    return 2;
  }
  const bool f32 = argc > 4 && std::strcmp(argv[4], "f32") == 0;
  std::map<Key, uint64_t> want;
  if (!read_expect(argv[3], &want)) {
    std::fprintf(stderr, "cannot read %s\n", argv[3]);
    return 2;
  }
  try {
    host_tests(argv[2], want, f32);
    if (std::strcmp(argv[1], "gpu") == 0) gpu_tests(argv[2], want, f32);
  } catch (const psg::Error& e) {
    std::fprintf(stderr, "psg::Error %d: %s\n", e.status(), e.what());
    return 1;
  }
  if (failures) std::fprintf(stderr, "%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
