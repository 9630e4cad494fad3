// TEST INFRASTRUCTURE ONLY.  Stand-in for the reference's
// system/postoffice.h: parameter/frequency_filter.h includes it and uses
// nothing from it.  It holds no arithmetic or control flow of a pinned
// function.
#pragma once
#include "util/common.h"
