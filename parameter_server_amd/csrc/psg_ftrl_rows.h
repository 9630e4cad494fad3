// psg_ftrl_rows.h -- the multi-model FTRL table (psg_ftrlm_*, include/psg.h):
// what psg_ftrl_rows.hip (kernels) and psg_ctx_ftrlm.hip (the context's side)
// share.  m models per key, 1 <= m <= PSG_FTRL_MAX_MODELS.
//
// Layout.  An index of 16-B slots {key, row}, eight to a 128-B line, slot =
// fmix64(key) & mask with linear probing; a slot is claimed by a 64-bit
// compare-and-swap of its key word from 0 and never freed.  Beside it the row
// store: cnt[row] = {pos, neg}, w[row][m], z[row][m], row-major.  Row ids are
// handed out in claim order (one integer atomic per wave); row 0 is key 0's,
// so every uint64 is a legal key and a slot whose row word is still 0 holds no
// row.  Growth rebuilds the index only and copies the row store as it is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psg.h"
#include "psg_internal.h"

namespace psg {

constexpr int kFtrlmMax = PSG_FTRL_MAX_MODELS;
constexpr int kFtrlmSlots = 64;   // counter lines: kFtrlmMax nnz words each
constexpr int kFtrlmParts = 256;  // norm partials: workgroups of the reduction
constexpr uint64_t kFtrlmNoRow = ~0ull;

struct FtrlmSlot {
  uint64_t key, row;
};
struct FtrlmHead {
  unsigned long long verdict;       // order violations of the message in flight
  unsigned long long err;           // rejected messages not yet reported
  unsigned long long overflow;      // keys that found no slot or row (never, by the load limit)
  unsigned long long zero_present;  // key 0 has been pushed (its row is row 0)
  unsigned long long rows_used;     // rows handed out: ids 1 .. rows_used
  unsigned long long export_n;
  unsigned long long pad[2];
  FtrlParam P[kFtrlmMax];
  unsigned long long nnz_res[kFtrlmMax];
  double norm_res[2 * kFtrlmMax];  // [2 j] = sum |w|, [2 j + 1] = sum w^2 of model j
  unsigned long long nnz_slots[kFtrlmSlots * kFtrlmMax];
  double partial[kFtrlmParts * 2 * kFtrlmMax];
};
struct FtrlmTable {
  FtrlmSlot* idx;
  uint64_t mask;  // slots - 1 (a power of two)
  uint64_t* cnt;  // [row_cap][2]
  double* w;      // [row_cap][m]
  double* z;
  uint64_t row_cap;
  FtrlmHead* head;
  uint32_t m;
  uint32_t gs;  // log2 G, G = the power of two >= m: the lanes that own one key
};

// log2 of the power of two >= m: the lanes that own one key (here) or one
// row or key of the minibatch (psg_worker_rows.hip)
inline uint32_t group_shift(int m) {
  uint32_t gs = 0;
  while ((1 << gs) < m) ++gs;
  return gs;
}

// one message: order check, then the update of all m models of every key,
// which applies nothing unless the check passed (a rejected message also
// counts in head->err).  grad[n][m].
hipError_t launch_ftrlm_push(const FtrlmTable& T, const uint64_t* keys, const uint32_t* pos,
                             const uint32_t* neg, const double* grad, uint64_t n, hipStream_t s);
// out[n][m]: the w rows, +0.0 for an absent key
hipError_t launch_ftrlm_pull(const FtrlmTable& T, const uint64_t* keys, uint64_t n, double* out,
                             hipStream_t s);
// any output may be null; w[n][m], z[n][m]
hipError_t launch_ftrlm_lookup(const FtrlmTable& T, const uint64_t* keys, uint64_t n,
                               uint64_t* pos, uint64_t* neg, double* w, double* z, uint8_t* found,
                               hipStream_t s);
// every slot of `from`'s index into `to`'s (zeroed; the same head and row ids)
hipError_t launch_ftrlm_rehash(const FtrlmTable& from, const FtrlmTable& to, hipStream_t s);
// head->nnz_res[j] = the sum of model j's counter slots ...
hipError_t launch_ftrlm_count(const FtrlmTable& T, hipStream_t s);
// ... and head->norm_res as well
hipError_t launch_ftrlm_status(const FtrlmTable& T, hipStream_t s);
// (key, w) of model j's nonzero weights, the first cap of them; head->export_n = their count
hipError_t launch_ftrlm_export(const FtrlmTable& T, int j, uint64_t* keys, double* w, uint64_t cap,
                               hipStream_t s);

// ---- checkpoint and restore ------------------------------
// Upsert of n whole entries keys[n], pos[n], neg[n], w[n][m], z[n][m]: the
// order check, then every key's counts and both rows replaced; applies nothing
// unless the check passed.
hipError_t launch_ftrlm_import(const FtrlmTable& T, const uint64_t* keys, const uint64_t* pos,
                               const uint64_t* neg, const double* w, const double* z, uint64_t n,
                               hipStream_t s);
// The same for one column: w[row][j] of every key; a fresh row is zeros elsewhere.
hipError_t launch_ftrlm_import_weights(const FtrlmTable& T, int j, const uint64_t* keys,
                                       const double* w, uint64_t n, hipStream_t s);
// Whole-state export in two steps, with the host's one wait between them.
// Step 1: small[0] = OR, small[1] = AND, small[2] = count of the keys that hold
// a row and lie in [lo, hi]; tile_sum (ftrlm_state_count_words words) is left
// as step 2's tile bases.  PSG_ERR_SIZE for an index of 2^32 - 1 slots or more.
size_t ftrlm_state_count_words(const FtrlmTable& T);
int launch_ftrlm_state_count(const FtrlmTable& T, uint64_t lo, uint64_t hi, uint32_t* tile_sum,
                             unsigned long long* small, hipStream_t s);
// Step 2: those n entries sorted by key into keys[n], pos[n], neg[n], w[n][m],
// z[n][m] (any may be null); differ = OR ^ AND; work: ftrlm_state_work_bytes(n).
size_t ftrlm_state_work_bytes(uint64_t n);
int launch_ftrlm_state(const FtrlmTable& T, uint64_t lo, uint64_t hi, uint64_t n, uint64_t differ,
                       const uint32_t* tile_base, void* work, uint64_t* keys, uint64_t* pos,
                       uint64_t* neg, double* w, double* z, hipStream_t s);

}  // namespace psg
