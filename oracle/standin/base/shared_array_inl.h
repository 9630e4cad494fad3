// TEST INFRASTRUCTURE ONLY.  Stand-in for the reference's
// base/shared_array_inl.h: the stand-in SArray is defined whole in
// base/shared_array.h.  It holds no arithmetic or control flow of a pinned
// function.
#pragma once
#include "base/shared_array.h"
