// TEST INFRASTRUCTURE ONLY.  C entry points onto the reference's own
// FreqencyFilter<uint64> over CountMin<uint64, uint8> (reference
// src/parameter/frequency_filter.h, src/base/countmin.h), compiled in place
// from the reference tree by oracle/Makefile into oracle/_ref/.
// oracle/standin/ supplies SArray and the CHECK macros.  Used by
// tools/record_reference.py and tests/test_reference_pin.py to pin the
// CountMin restatements (oracle/psg_oracle.c, tests/test_freq_filter.py).
//
// PINNED here: resize, clear, empty, insertKeys, queryKeys and, below them,
// CountMin's hash, insert and query.  OURS: reading the table (count_ and
// data_ are private, so the two headers are included with private opened;
// nothing of them is re-implemented) and SArray's members.
#include "util/common.h"
#define private public
#include "parameter/frequency_filter.h"
#undef private

using namespace PS;

extern "C" {

void* ref_ff_create() { return new FreqencyFilter<uint64>(); }
void ref_ff_destroy(void* h) { delete (FreqencyFilter<uint64>*)h; }
void ref_ff_resize(void* h, int n, int k) {
  ((FreqencyFilter<uint64>*)h)->resize(n, k);
}
void ref_ff_clear(void* h) { ((FreqencyFilter<uint64>*)h)->clear(); }
int ref_ff_empty(void* h) { return ((FreqencyFilter<uint64>*)h)->empty(); }

void ref_ff_insert_keys(void* h, const uint64* keys, const uint32* counts,
                        size_t n) {
  SArray<uint64> k(n);
  SArray<uint32> c(n);
  if (n) {
    memcpy(k.data(), keys, n * sizeof(uint64));
    memcpy(c.data(), counts, n * sizeof(uint32));
  }
  ((FreqencyFilter<uint64>*)h)->insertKeys(k, c);
}

// out holds n keys; returns how many were kept
size_t ref_ff_query_keys(void* h, const uint64* keys, size_t n, int freq,
                         uint64* out) {
  SArray<uint64> k(n);
  if (n) memcpy(k.data(), keys, n * sizeof(uint64));
  SArray<uint64> kept = ((FreqencyFilter<uint64>*)h)->queryKeys(k, freq);
  if (kept.size()) memcpy(out, kept.data(), kept.size() * sizeof(uint64));
  return kept.size();
}

// the table: n_, k_ and data_'s bytes (out == NULL only reports the sizes)
void ref_ff_table(void* h, int* n, int* k, unsigned char* out) {
  auto& cm = ((FreqencyFilter<uint64>*)h)->count_;
  *n = cm.n_;
  *k = cm.k_;
  if (out && cm.data_.size()) memcpy(out, cm.data_.data(), cm.data_.size());
}

}  // extern "C"
