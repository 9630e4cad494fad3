// psg_ctx_ftrl.hip -- the FTRL model of a context (FTRLModel<uint64, double>:
// psg_ftrl_*, include/psg.h) over the hash-table kernels of psg_ftrl.hip.
#include "psg_ctx.h"

extern "C" {

// ------------------------------------------------------------ FTRL model --
namespace {

int ftrl_order(Ftrl* F, hipStream_t s) {
  if (F->last && F->last_s != s) HIP_TRY(hipStreamWaitEvent(s, F->last, 0));
  return PSG_OK;
}
int ftrl_mark(psg_ctx* c, Ftrl* F, hipStream_t s) {
  if (!F->last)
    if (int rc = c->event(&F->last)) return rc;
  HIP_TRY(hipEventRecord(F->last, s));
  F->last_s = s;
  return PSG_OK;
}

int ftrl_of(psg_ctx* c, Ftrl** F) {
  if (!c->ftrl.on) return fail(PSG_ERR_ARG, "no FTRL model (psg_ftrl_init)");
  *F = &c->ftrl;
  return PSG_OK;
}

// A zeroed table of nb buckets on the context's stream.
int ftrl_table(psg_ctx* c, uint64_t nb, psg::FtrlBucket** out) {
  if (int rc = c->dev_get(sizeof(psg::FtrlBucket) * nb, (void**)out, c->stream)) return rc;
  HIP_TRY(hipMemsetAsync(*out, 0, sizeof(psg::FtrlBucket) * nb, c->stream));
  return PSG_OK;
}

// Every entry moves into a table of nb buckets, on the context's stream and
// in the model's call order; no host wait.
int ftrl_grow(psg_ctx* c, Ftrl* F, uint64_t nb) {
  psg::FtrlBucket* nt = nullptr;
  if (int rc = ftrl_order(F, c->stream)) return rc;
  if (int rc = ftrl_table(c, nb, &nt)) return rc;
  const psg::FtrlTable from = F->table(), to{nt, nb - 1, F->d_head};
  const hipError_t e = psg::launch_ftrl_rehash(from, to, c->stream);
  if (e != hipSuccess) {
    c->dev_put(nt, sizeof(psg::FtrlBucket) * nb);
    return fail(PSG_ERR_DEVICE, "ftrl rehash: %s", hipGetErrorString(e));
  }
  c->dev_put(F->d_tab, sizeof(psg::FtrlBucket) * F->nb);
  F->d_tab = nt;
  F->nb = nb;
  return ftrl_mark(c, F, c->stream);
}

// Room for n more keys.  The common case is host arithmetic on the bound;
// only when the bound would pass the load limit is the true entry count read
// from the device (a wait), and only if that still does not fit does the
// table grow.
int ftrl_room(psg_ctx* c, Ftrl* F, size_t n) {
  if (F->bound + n > F->limit()) {
    if (int rc = ftrl_order(F, c->stream)) return rc;
    HIP_TRY(psg::launch_ftrl_count(F->table(), c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_small + 8, F->d_head->res, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    F->bound = (size_t)c->h_small[8];
    if (F->bound + n > F->limit()) {
      const uint64_t nb = std::max(2 * F->nb, Ftrl::buckets_for(F->bound + n));
      if (int rc = ftrl_grow(c, F, nb)) return rc;
    }
  }
  F->bound += n;
  return PSG_OK;
}

// A message that was not strictly increasing is reported once, by the next
// call that waits for the device (`rejected`: head->err as just read there).
int ftrl_report(psg_ctx* c, Ftrl* F, unsigned long long rejected) {
  if (!rejected) return PSG_OK;
  HIP_TRY(hipMemsetAsync(&F->d_head->err, 0, 8, c->stream));
  if (int rc = ftrl_mark(c, F, c->stream)) return rc;
  return fail(PSG_ERR_UNSORTED, "%llu key pairs of FTRL pushes not strictly increasing: "
              "those messages were not applied", rejected);
}

// a push into an evaluation-only model (psg_ftrl_import's weights-only form)
int ftrl_unfrozen(Ftrl* F) {
  if (F->frozen)
    return fail(PSG_ERR_ARG, "the FTRL model is frozen: it was loaded by a weights-only import "
                "(evaluation only), z is unknown and a push would recompute w from it");
  return PSG_OK;
}

// pos, neg and z of an import: all given, or all null (the weights-only form)
int import_form(const void* pos, const void* neg, const void* z, bool* weights_only) {
  const int nulls = !pos + !neg + !z;
  if (nulls != 0 && nulls != 3)
    return fail(PSG_ERR_ARG, "FTRL import: pos, neg and z are all given or all NULL");
  *weights_only = nulls == 3;
  return PSG_OK;
}

// the device words and pinned host words of a state export
constexpr int kStateWords = 20;  // h_small[20..23]: OR, AND, count, err

// Step 1 of a state export on stream s: *blk (state_count_bytes) holds the
// three device words and, from byte 64, the scan's tile sums; the host then
// knows the count, the key bits that differ and the rejected messages.  Waits.
size_t state_count_bytes(Ftrl* F) { return 64 + 4 * psg::ftrl_state_count_words(F->table()); }
int state_count(psg_ctx* c, Ftrl* F, uint64_t lo, uint64_t hi, hipStream_t s, char** blk,
                size_t* n, uint64_t* differ, unsigned long long* rejected) {
  if (int rc = ftrl_order(F, s)) return rc;
  if (int rc = c->dev_get(state_count_bytes(F), (void**)blk, s)) return rc;
  unsigned long long* small = (unsigned long long*)*blk;
  unsigned long long* h = c->h_small + kStateWords;
  if (int rc = psg::launch_ftrl_state_count(F->table(), lo, hi, (uint32_t*)(*blk + 64), small, s))
    return rc;
  HIP_TRY(hipMemcpyAsync(h, small, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h + 3, &F->d_head->err, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n = (size_t)(h[2] & 0xffffffffull);
  *differ = h[0] ^ h[1];
  *rejected = h[3];
  return PSG_OK;
}

// a block used on stream s goes back to the pool, whose release events are
// recorded on the context's stream: that stream first waits for the model's
// last event (recorded on s after the block's last use)
void state_put(psg_ctx* c, Ftrl* F, hipStream_t s, void* blk, size_t bytes) {
  if (!blk) return;
  if (s != c->stream && F->last) (void)hipStreamWaitEvent(c->stream, F->last, 0);
  c->dev_put(blk, bytes);
}

// Step 2: the n entries of [lo, hi] sorted by key into device arrays.
int state_emit(psg_ctx* c, Ftrl* F, uint64_t lo, uint64_t hi, size_t n, uint64_t differ,
               const char* count_blk, uint64_t* keys, uint64_t* pos, uint64_t* neg, double* w,
               double* z, hipStream_t s) {
  if (n == 0) return PSG_OK;
  const size_t wb = psg::ftrl_state_work_bytes(n);
  void* work = nullptr;
  if (int rc = c->dev_get(wb, &work, s)) return rc;
  int rc = psg::launch_ftrl_state(F->table(), lo, hi, n, differ,
                                  (const uint32_t*)(count_blk + 64), work, keys, pos, neg, w, z, s);
  const int rm = ftrl_mark(c, F, s);
  state_put(c, F, s, work, wb);
  return rc ? rc : rm;
}

int state_range(const uint64_t* range, uint64_t* lo, uint64_t* hi) {
  *lo = range ? range[0] : 0;
  *hi = range ? range[1] : ~0ull;
  if (*lo > *hi) return fail(PSG_ERR_ARG, "FTRL state export: range[0] > range[1]");
  return PSG_OK;
}

}  // namespace

int psg_ftrl_init(psg_ctx* c, const psg_ftrl_param* p, size_t capacity_hint) {
  if (!c || !p) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  if (c->dtype != PSG_F64) return fail(PSG_ERR_ARG, "FTRL needs a PSG_F64 context");
  if (int rc = set_dev(c->device)) return rc;
  ftrl_release(c);
  Ftrl& F = c->ftrl;
  const uint64_t nb = Ftrl::buckets_for(capacity_hint ? capacity_hint : (size_t(1) << 20));
  if (int rc = c->dev_get(sizeof(psg::FtrlHead), (void**)&F.d_head, c->stream)) return rc;
  int rc = ftrl_table(c, nb, &F.d_tab);
  if (rc == PSG_OK &&
      hipMemsetAsync(F.d_head, 0, sizeof(psg::FtrlHead), c->stream) != hipSuccess)
    rc = fail(PSG_ERR_DEVICE, "ftrl init");
  if (rc != PSG_OK) {
    ftrl_release(c);
    return rc;
  }
  F.nb = nb;
  F.P = psg::FtrlParam{p->alpha, p->beta, p->lambda1, p->lambda2};
  F.on = true;
  return ftrl_mark(c, &F, c->stream);
}

int psg_ftrl_reserve(psg_ctx* c, size_t entries) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (entries <= F->limit()) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  return ftrl_grow(c, F, Ftrl::buckets_for(entries));
}

int psg_ftrl_push_dev(psg_ctx* c, const uint64_t* keys, size_t n, const uint32_t* pos,
                      const uint32_t* neg, const double* grad, void* stream) {
  if (!c || (n && (!keys || !pos || !neg || !grad))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (int rc = ftrl_unfrozen(F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrl_room(c, F, n)) return rc;
  if (int rc = ftrl_order(F, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_ftrl_push(F->table(), keys, pos, neg, grad, n, F->P, (hipStream_t)stream));
  return ftrl_mark(c, F, (hipStream_t)stream);
}

int psg_ftrl_push(psg_ctx* c, const uint64_t* keys, size_t n, const uint32_t* pos,
                  const uint32_t* neg, const double* grad) {
  if (!c || (n && (!keys || !pos || !neg || !grad))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (int rc = ftrl_unfrozen(F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrl_room(c, F, n)) return rc;
  // one staging block for the four arrays, back to the pool after the kernels
  const size_t kb = align_up(8 * n, 256), cb = align_up(4 * n, 256), b = 2 * kb + 2 * cb;
  char* blk = nullptr;
  if (int rc = c->dev_get(b, (void**)&blk, c->copy)) return rc;
  int rc = c->h2d(blk, keys, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + kb, grad, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + 2 * kb, pos, 4 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + 2 * kb + cb, neg, 4 * n);
  if (rc == PSG_OK) rc = c->join_copy();
  if (rc == PSG_OK) rc = ftrl_order(F, c->stream);
  if (rc == PSG_OK) {
    const hipError_t e = psg::launch_ftrl_push(
        F->table(), (const uint64_t*)blk, (const uint32_t*)(blk + 2 * kb),
        (const uint32_t*)(blk + 2 * kb + cb), (const double*)(blk + kb), n, F->P, c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "ftrl push: %s", hipGetErrorString(e));
  }
  if (rc == PSG_OK) rc = ftrl_mark(c, F, c->stream);
  c->dev_put(blk, b);
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

int psg_ftrl_pull_dev(psg_ctx* c, const uint64_t* keys, size_t n, double* out, void* stream) {
  if (!c || (n && (!keys || !out))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = ftrl_order(F, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_ftrl_pull(F->table(), keys, n, out, (hipStream_t)stream));
  return ftrl_mark(c, F, (hipStream_t)stream);
}

int psg_ftrl_pull(psg_ctx* c, const uint64_t* keys, size_t n, double* out) {
  if (!c || (n && (!keys || !out))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  const size_t kb = align_up(8 * n, 256);
  if (int rc = c->ensure_scratch(2 * kb)) return rc;
  uint64_t* d_keys = (uint64_t*)c->scratch;
  double* d_out = (double*)((char*)c->scratch + kb);
  if (int rc = c->h2d(d_keys, keys, 8 * n)) return rc;
  if (int rc = c->join_copy()) return rc;
  if (int rc = ftrl_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_ftrl_pull(F->table(), d_keys, n, d_out, c->stream));
  if (int rc = ftrl_mark(c, F, c->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, 8 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small + 9, &F->d_head->err, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (int rc = c->h2d_finish()) return rc;
  return ftrl_report(c, F, c->h_small[9]);
}

int psg_ftrl_status(psg_ctx* c, size_t* entries, size_t* nnz, double* norm1, double* norm2) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrl_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_ftrl_norm(F->table(), c->stream));
  if (int rc = ftrl_mark(c, F, c->stream)) return rc;
  // verdict .. overflow, then res[0..3]
  HIP_TRY(hipMemcpyAsync(c->h_small + 8, F->d_head, 24, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small + 12, F->d_head->res, 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->h_small[10])  // unreachable while the load limit holds
    return fail(PSG_ERR_DEVICE, "FTRL table full: %llu keys were dropped", c->h_small[10]);
  F->bound = (size_t)c->h_small[12];
  if (entries) *entries = (size_t)c->h_small[12];
  if (nnz) *nnz = (size_t)c->h_small[13];
  if (norm1) memcpy(norm1, c->h_small + 14, 8);
  if (norm2) memcpy(norm2, c->h_small + 15, 8);
  return ftrl_report(c, F, c->h_small[9]);
}

int psg_ftrl_export(psg_ctx* c, uint64_t* keys, double* w, size_t cap, size_t* n) {
  if (!c || !n || (cap && (!keys || !w))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (int rc = set_dev(c->device)) return rc;
  *n = 0;
  if (int rc = ftrl_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_ftrl_count(F->table(), c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small + 8, &F->d_head->err, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small + 12, F->d_head->res, 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const unsigned long long rejected = c->h_small[8];
  const size_t need = (size_t)c->h_small[13];
  *n = need;
  if (need > cap)
    return fail(PSG_ERR_SIZE, "FTRL export: %zu nonzero weights, room for %zu", need, cap);
  if (need) {
    const size_t kb = align_up(8 * need, 256);
    if (int rc = c->ensure_scratch(2 * kb)) return rc;
    uint64_t* d_keys = (uint64_t*)c->scratch;
    double* d_w = (double*)((char*)c->scratch + kb);
    HIP_TRY(psg::launch_ftrl_export(F->table(), d_keys, d_w, need, c->stream));
    if (int rc = ftrl_mark(c, F, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(keys, d_keys, 8 * need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(w, d_w, 8 * need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return ftrl_report(c, F, rejected);
}

int psg_ftrl_import_dev(psg_ctx* c, const uint64_t* keys, size_t n, const uint64_t* pos,
                        const uint64_t* neg, const double* w, const double* z, void* stream) {
  if (!c || (n && (!keys || !w))) return fail(PSG_ERR_ARG, "null argument");
  bool weights_only;
  if (int rc = import_form(pos, neg, z, &weights_only)) return rc;
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (n == 0) {  // an empty weights-only import (w given) still freezes
    if (weights_only && w) F->frozen = true;
    return PSG_OK;
  }
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrl_room(c, F, n)) return rc;
  if (int rc = ftrl_order(F, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_ftrl_import(F->table(), keys, pos, neg, w, z, n, (hipStream_t)stream));
  if (weights_only) F->frozen = true;
  return ftrl_mark(c, F, (hipStream_t)stream);
}

int psg_ftrl_import(psg_ctx* c, const uint64_t* keys, size_t n, const uint64_t* pos,
                    const uint64_t* neg, const double* w, const double* z) {
  if (!c || (n && (!keys || !w))) return fail(PSG_ERR_ARG, "null argument");
  bool weights_only;
  if (int rc = import_form(pos, neg, z, &weights_only)) return rc;
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (n == 0) {  // an empty weights-only import (w given) still freezes
    if (weights_only && w) F->frozen = true;
    return PSG_OK;
  }
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrl_room(c, F, n)) return rc;
  // one staging block for the arrays, back to the pool after the kernels
  const size_t kb = align_up(8 * n, 256), b = (weights_only ? 2 : 5) * kb;
  char* blk = nullptr;
  if (int rc = c->dev_get(b, (void**)&blk, c->copy)) return rc;
  int rc = c->h2d(blk, keys, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + kb, w, 8 * n);
  if (rc == PSG_OK && !weights_only) rc = c->h2d(blk + 2 * kb, pos, 8 * n);
  if (rc == PSG_OK && !weights_only) rc = c->h2d(blk + 3 * kb, neg, 8 * n);
  if (rc == PSG_OK && !weights_only) rc = c->h2d(blk + 4 * kb, z, 8 * n);
  if (rc == PSG_OK) rc = c->join_copy();
  if (rc == PSG_OK) rc = ftrl_order(F, c->stream);
  if (rc == PSG_OK) {
    const hipError_t e = psg::launch_ftrl_import(
        F->table(), (const uint64_t*)blk, weights_only ? nullptr : (const uint64_t*)(blk + 2 * kb),
        weights_only ? nullptr : (const uint64_t*)(blk + 3 * kb), (const double*)(blk + kb),
        weights_only ? nullptr : (const double*)(blk + 4 * kb), n, c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "ftrl import: %s", hipGetErrorString(e));
  }
  if (rc == PSG_OK && weights_only) F->frozen = true;
  if (rc == PSG_OK) rc = ftrl_mark(c, F, c->stream);
  c->dev_put(blk, b);
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

int psg_ftrl_frozen(psg_ctx* c, int* frozen) {
  if (!c || !frozen) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  *frozen = F->frozen ? 1 : 0;
  return PSG_OK;
}

int psg_ftrl_export_state_dev(psg_ctx* c, const uint64_t* range, uint64_t* keys, uint64_t* pos,
                              uint64_t* neg, double* w, double* z, size_t cap,
                              unsigned long long* n_dev, void* stream) {
  if (!c || !n_dev) return fail(PSG_ERR_ARG, "null argument");
  uint64_t lo, hi;
  if (int rc = state_range(range, &lo, &hi)) return rc;
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (int rc = set_dev(c->device)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* cb = nullptr;
  const size_t cbytes = state_count_bytes(F);
  size_t n = 0;
  uint64_t differ = 0;
  unsigned long long rejected = 0;
  int rc = state_count(c, F, lo, hi, s, &cb, &n, &differ, &rejected);
  if (rc == PSG_OK && hipMemcpyAsync(n_dev, cb + 16, 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
    rc = fail(PSG_ERR_DEVICE, "ftrl state export: count copy");
  if (rc == PSG_OK && n > cap)
    rc = fail(PSG_ERR_SIZE, "FTRL state export: %zu entries, room for %zu", n, cap);
  else if (rc == PSG_OK)
    rc = state_emit(c, F, lo, hi, n, differ, cb, keys, pos, neg, w, z, s);
  const int rm = ftrl_mark(c, F, s);
  state_put(c, F, s, cb, cbytes);
  return rc ? rc : rm;
}

int psg_ftrl_export_state(psg_ctx* c, const uint64_t* range, uint64_t* keys, uint64_t* pos,
                          uint64_t* neg, double* w, double* z, size_t cap, size_t* n_out) {
  if (!c || !n_out) return fail(PSG_ERR_ARG, "null argument");
  uint64_t lo, hi;
  if (int rc = state_range(range, &lo, &hi)) return rc;
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (int rc = set_dev(c->device)) return rc;
  *n_out = 0;
  hipStream_t s = c->stream;
  char* cb = nullptr;
  const size_t cbytes = state_count_bytes(F);
  size_t n = 0;
  uint64_t differ = 0;
  unsigned long long rejected = 0;
  int rc = state_count(c, F, lo, hi, s, &cb, &n, &differ, &rejected);
  if (rc == PSG_OK) *n_out = n;
  if (rc == PSG_OK && n > cap)
    rc = fail(PSG_ERR_SIZE, "FTRL state export: %zu entries, room for %zu", n, cap);
  void* const dst[5] = {keys, pos, neg, w, z};
  const bool any = keys || pos || neg || w || z;
  if (rc == PSG_OK && n && any) {
    const size_t kb = align_up(8 * n, 256);
    char* ob = nullptr;
    rc = c->dev_get(5 * kb, (void**)&ob, s);
    if (rc == PSG_OK) {
      void* d[5];
      for (int i = 0; i < 5; ++i) d[i] = dst[i] ? ob + i * kb : nullptr;
      rc = state_emit(c, F, lo, hi, n, differ, cb, (uint64_t*)d[0], (uint64_t*)d[1],
                      (uint64_t*)d[2], (double*)d[3], (double*)d[4], s);
      for (int i = 0; i < 5 && rc == PSG_OK; ++i)
        if (dst[i] &&
            hipMemcpyAsync(dst[i], d[i], 8 * n, hipMemcpyDeviceToHost, s) != hipSuccess)
          rc = fail(PSG_ERR_DEVICE, "ftrl state export: copy to the host");
      if (hipStreamSynchronize(s) != hipSuccess && rc == PSG_OK)
        rc = fail(PSG_ERR_DEVICE, "ftrl state export: wait");
      c->dev_put(ob, 5 * kb);
    }
  }
  c->dev_put(cb, cbytes);
  if (rc != PSG_OK) return rc;
  return ftrl_report(c, F, rejected);
}

int psg_ftrl_lookup(psg_ctx* c, const uint64_t* keys, size_t n, uint64_t* pos, uint64_t* neg,
                    double* w, double* z, uint8_t* found) {
  if (!c || (n && !keys)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrl* F;
  if (int rc = ftrl_of(c, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  const size_t kb = align_up(8 * n, 256);
  if (int rc = c->ensure_scratch(6 * kb)) return rc;
  char* s = (char*)c->scratch;
  if (int rc = c->h2d(s, keys, 8 * n)) return rc;
  if (int rc = c->join_copy()) return rc;
  if (int rc = ftrl_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_ftrl_lookup(F->table(), (const uint64_t*)s, n, (uint64_t*)(s + kb),
                                  (uint64_t*)(s + 2 * kb), (double*)(s + 3 * kb),
                                  (double*)(s + 4 * kb), (uint8_t*)(s + 5 * kb), c->stream));
  if (int rc = ftrl_mark(c, F, c->stream)) return rc;
  void* const dst[5] = {pos, neg, w, z, found};
  for (int i = 0; i < 5; ++i)
    if (dst[i])
      HIP_TRY(hipMemcpyAsync(dst[i], s + (i + 1) * kb, i < 4 ? 8 * n : n, hipMemcpyDeviceToHost,
                             c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return c->h2d_finish();
}

}  // extern "C"

void psg::ftrl_release(psg_ctx* c) {
  Ftrl& F = c->ftrl;
  if (F.last) {
    (void)hipEventSynchronize(F.last);
    c->free_ev.push_back(F.last);
    F.last = nullptr;
  }
  // the pool's release events are recorded on the context's stream, which
  // is past every operation of the model once their last event completed
  c->dev_put(F.d_tab, sizeof(psg::FtrlBucket) * F.nb);
  c->dev_put(F.d_head, sizeof(psg::FtrlHead));
  F = Ftrl();
}
