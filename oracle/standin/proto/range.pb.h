// TEST INFRASTRUCTURE ONLY.  Stand-in for the protobuf-generated PbRange
// (a begin/end pair with accessors), written for oracle/ref_*_shim.cc from
// what the reference's base/range.h calls.  It holds no arithmetic or
// control flow of a pinned function.
#pragma once
#include "util/common.h"

namespace PS {
struct PbRange {
  uint64 b = 0, e = 0;
  uint64 begin() const { return b; }
  uint64 end() const { return e; }
  void set_begin(uint64 v) { b = v; }
  void set_end(uint64 v) { e = v; }
};
}  // namespace PS
