// MEASUREMENT AID of tools/ftrl_bench.py: the FTRL server update on one CPU
// core over std::unordered_map, the container the reference's model uses.
// Written from the contract in include/psg.h (psg_ftrl_push / psg_ftrl_pull);
// not product code and not a test oracle (tests/ftrl_ref.py is).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <unordered_map>

namespace {

struct Entry {
  uint64_t pos = 0, neg = 0;
  double w = 0, z = 0;
};

struct Model {
  double alpha, beta, lambda1, lambda2;
  std::unordered_map<uint64_t, Entry> map;
  size_t nnz = 0;
};

inline double count_norm(uint64_t pos, uint64_t neg) {
  const double p = (double)pos, n = (double)neg, all = p + n;
  return all == 0 ? 0 : std::sqrt(p * n / all);
}

}  // namespace

extern "C" {

void* ftrl_cpu_new(double alpha, double beta, double lambda1, double lambda2, size_t reserve) {
  Model* m = new Model{alpha, beta, lambda1, lambda2, {}, 0};
  m->map.reserve(reserve);
  return m;
}

void ftrl_cpu_free(void* h) { delete (Model*)h; }

size_t ftrl_cpu_size(void* h) { return ((Model*)h)->map.size(); }
size_t ftrl_cpu_nnz(void* h) { return ((Model*)h)->nnz; }

void ftrl_cpu_push(void* h, const uint64_t* keys, size_t n, const uint32_t* pos,
                   const uint32_t* neg, const double* grad) {
  Model& m = *(Model*)h;
  for (size_t i = 0; i < n; ++i) {
    Entry& e = m.map[keys[i]];
    const double before = count_norm(e.pos, e.neg);
    e.pos += pos[i];
    e.neg += neg[i];
    const double after = count_norm(e.pos, e.neg);
    e.z += grad[i] - (after - before) / m.alpha * e.w;
    const double l2 = m.lambda2 + (m.beta + after) / m.alpha;
    double t = 0;
    if (e.z > m.lambda1) t = (e.z - m.lambda1) / l2;
    if (e.z < -m.lambda1) t = (e.z + m.lambda1) / l2;
    const double w = -t;
    m.nnz += (w != 0) - (e.w != 0);
    e.w = w;
  }
}

void ftrl_cpu_pull(void* h, const uint64_t* keys, size_t n, double* out) {
  Model& m = *(Model*)h;
  for (size_t i = 0; i < n; ++i) {
    auto it = m.map.find(keys[i]);
    out[i] = it == m.map.end() ? 0.0 : it->second.w;
  }
}

}  // extern "C"
