// TEST INFRASTRUCTURE ONLY.  Stand-in for the reference's
// parameter/shared_parameter.h, written for oracle/ref_ftrl_shim.cc: an
// empty SharedParameter base for FTRLModel to derive from.  Message and
// sliceKeyOrderedMsg come from the reference's own system/message.h.  It
// holds no arithmetic or control flow of a pinned function.
#pragma once
#include "system/message.h"

namespace PS {
template <typename K> class SharedParameter {
 public:
  virtual ~SharedParameter() {}
};
}  // namespace PS
