// TEST INFRASTRUCTURE ONLY.  Stand-in for glog's logging.h, written for
// oracle/ref_*_shim.cc from what the reference's call sites need: CHECK*
// macros that abort on failure and swallow what is streamed into them.
// It holds no arithmetic or control flow of a pinned function.
#pragma once
#include <stdlib.h>

namespace standin {
struct Sink {
  bool fatal;
  ~Sink() { if (fatal) abort(); }
  template <typename T> Sink& operator<<(const T&) { return *this; }
};
}  // namespace standin

#define CHECK(x) if (x) {} else ::standin::Sink{true}
#define CHECK_EQ(a, b) CHECK((a) == (b))
#define CHECK_NE(a, b) CHECK((a) != (b))
#define CHECK_GT(a, b) CHECK((a) > (b))
#define CHECK_LT(a, b) CHECK((a) < (b))
#define CHECK_GE(a, b) CHECK((a) >= (b))
#define CHECK_LE(a, b) CHECK((a) <= (b))
