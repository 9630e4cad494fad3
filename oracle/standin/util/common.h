// TEST INFRASTRUCTURE ONLY.  Stand-in for the reference's util/common.h,
// written for oracle/ref_*_shim.cc from what the pinned headers need of it:
// the standard headers, the integer typedefs (the reference's own
// util/integral_types.h), Key/KeyList, the error-log stream LL and the
// num_threads flag as a plain int.  It holds no arithmetic or control flow
// of a pinned function.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <functional>
#include <initializer_list>
#include <iostream>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "glog/logging.h"
#include "util/integral_types.h"
#include "util/macros.h"

#define LL ::standin::Sink{false}

// gflags' --num_threads; each shim defines and sets it per call
extern int FLAGS_num_threads;

namespace PS {
typedef uint64 Key;
typedef std::vector<Key> KeyList;
}  // namespace PS
