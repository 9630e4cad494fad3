// C++ driver for the FTRLModel adapter (parameter_server_amd/csrc/ftrl_model.h),
// built with plain g++ against libpsg.so.  Reads like the reference's server
// side: a model gets its learning rate and penalty, receives messages
// (setValue), answers a pull (getValue) and dumps itself.  The messages and
// the expected bits come from a file the Python side wrote from its
// restatement (tests/ftrl_ref.py):
//   P alpha beta lambda1 lambda2          (doubles as hex bit patterns)
//   M n      then n lines: key pos neg grad-bits
//   G n      then n lines: key w-bits     (the expected pull)
//   S nnz    the expected nnz
//   D n      then n lines of the expected dump text
//
//   test_ftrl_model host FILE  -- parse only (no GPU)
//   test_ftrl_model gpu FILE   -- the model on device 0
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include <unistd.h>

#include "../../parameter_server_amd/csrc/ftrl_model.h"

using psg::Key;
using psg::Message;
using psg::MessagePtr;

static int failures = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: EXPECT(%s)\n", __FILE__, __LINE__, #c); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static double from_bits(uint64_t b) {
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}
static uint64_t to_bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

struct Case {
  double param[4];
  std::vector<MessagePtr> msgs;
  std::vector<Key> pull_keys;
  std::vector<uint64_t> pull_bits;
  size_t nnz = 0;
  std::string dump;
};

static bool read_case(const char* path, Case* c) {
  std::ifstream in(path);
  if (!in.good()) return false;
  std::string tag;
  while (in >> tag) {
    if (tag == "P") {
      for (int i = 0; i < 4; ++i) {
        uint64_t b;
        in >> std::hex >> b >> std::dec;
        c->param[i] = from_bits(b);
      }
    } else if (tag == "M") {
      size_t n;
      in >> n;
      MessagePtr m(new Message());
      std::vector<uint32_t> pos(n), neg(n);
      std::vector<double> grad(n);
      m->key.resize(n);
      for (size_t i = 0; i < n; ++i) {
        uint64_t g;
        in >> m->key[i] >> pos[i] >> neg[i] >> std::hex >> g >> std::dec;
        grad[i] = from_bits(g);
      }
      m->addValue(pos);
      m->addValue(neg);
      m->addValue(grad);
      c->msgs.push_back(m);
    } else if (tag == "G") {
      size_t n;
      in >> n;
      c->pull_keys.resize(n);
      c->pull_bits.resize(n);
      for (size_t i = 0; i < n; ++i)
        in >> c->pull_keys[i] >> std::hex >> c->pull_bits[i] >> std::dec;
    } else if (tag == "S") {
      in >> c->nnz;
    } else if (tag == "D") {
      size_t n;
      in >> n;
      std::string line;
      std::getline(in, line);
      for (size_t i = 0; i < n; ++i) {
        std::getline(in, line);
        c->dump += line + "\n";
      }
    } else {
      return false;
    }
  }
  return !in.bad();
}

static void gpu_tests(const Case& c) {
  psg::FTRLModel<double> model(0, 64);
  model.setLearningRate(c.param[0], c.param[1]);
  model.setPenalty(c.param[2], c.param[3]);
  for (const auto& m : c.msgs) model.setValue(m);

  MessagePtr req(new Message());
  req->key = c.pull_keys;
  model.getValue(req);
  EXPECT(req->value.size() == 1);
  const std::vector<double> w = req->valueAs<double>(0);
  EXPECT(w.size() == c.pull_bits.size());
  size_t bad = 0;
  for (size_t i = 0; i < w.size() && i < c.pull_bits.size(); ++i)
    bad += to_bits(w[i]) != c.pull_bits[i];
  EXPECT(bad == 0);
  EXPECT(model.nnz() == c.nnz);
  EXPECT(model.objv() > 0);

  const std::string path = std::string(std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp") +
                           "/psg_ftrl_dump_" + std::to_string((long)getpid()) + ".txt";
  model.writeToFile(path);
  std::ifstream f(path);
  std::stringstream got;
  got << f.rdbuf();
  EXPECT(got.str() == c.dump);
  std::remove(path.c_str());

  // the reference's CHECKs come back as psg::Error
  bool threw = false;
  try {
    MessagePtr m(new Message());
    m->key = {1, 2};
    m->addValue(std::vector<uint32_t>{1, 1});
    model.setValue(m);  // one value array, not three
  } catch (const psg::Error& e) {
    threw = e.status() == PSG_ERR_SIZE;
  }
  EXPECT(threw);
  threw = false;
  try {
    model.setPenalty(1, 1);  // after the first message
  } catch (const psg::Error& e) {
    threw = e.status() == PSG_ERR_ARG;
  }
  EXPECT(threw);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s host|gpu FILE\n", argv[0]);
    return 2;
  }
  Case c;
  if (!read_case(argv[2], &c)) {
    std::fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  EXPECT(c.msgs.size() == 3 && !c.pull_keys.empty() && !c.dump.empty());
  if (std::strcmp(argv[1], "gpu") == 0) {
    try {
      gpu_tests(c);
    } catch (const psg::Error& e) {
      std::fprintf(stderr, "psg::Error %d: %s\n", e.status(), e.what());
      return 1;
    }
  }
  if (failures) std::fprintf(stderr, "%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
