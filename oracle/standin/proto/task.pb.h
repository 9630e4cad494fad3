// TEST INFRASTRUCTURE ONLY.  Stand-in for the protobuf-generated Task and
// the three config messages the pinned headers read, written for
// oracle/ref_*_shim.cc from their call sites (plain structs with the
// accessors used).  It holds no arithmetic or control flow of a pinned
// function.
#pragma once
#include "proto/range.pb.h"

namespace PS {
struct Task {
  PbRange r;
  const PbRange& key_range() const { return r; }
  PbRange* mutable_key_range() { return &r; }
};
struct LearningRateConfig {
  double a = 0, b = 0;
  double alpha() const { return a; }
  double beta() const { return b; }
};
struct PenaltyConfig {
  std::vector<double> l;
  int lambda_size() const { return (int)l.size(); }
  double lambda(int i) const { return l[i]; }
};
struct DataConfig {
  std::vector<std::string> f;
  const std::string& file(int i) const { return f[i]; }
};
}  // namespace PS
