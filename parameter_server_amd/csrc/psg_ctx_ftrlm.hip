// psg_ctx_ftrlm.hip -- the multi-model FTRL of a context (psg_ftrlm_*,
// include/psg.h) over the kernels of psg_ftrl_rows.hip.  The contract is
// psg_ctx_ftrl.hip's: messages apply in call order whatever the stream, a push
// allocates nothing and waits for nothing while the model has room, and a
// rejected message is reported once by the next call that synchronises.
#include "psg_ctx.h"
#include "psg_score.h"

extern "C" {

namespace {

int ftrlm_order(Ftrlm* F, hipStream_t s) {
  if (F->last && F->last_s != s) HIP_TRY(hipStreamWaitEvent(s, F->last, 0));
  return PSG_OK;
}
int ftrlm_mark(psg_ctx* c, Ftrlm* F, hipStream_t s) {
  if (!F->last)
    if (int rc = c->event(&F->last)) return rc;
  HIP_TRY(hipEventRecord(F->last, s));
  F->last_s = s;
  return PSG_OK;
}

int ftrlm_of(psg_ctx* c, Ftrlm** F) {
  if (!c->ftrlm.on) return fail(PSG_ERR_ARG, "no multi-model FTRL (psg_ftrlm_init)");
  *F = &c->ftrlm;
  return PSG_OK;
}

// the index and the row store for `ns` slots
struct Store {
  psg::FtrlmSlot* idx = nullptr;
  uint64_t* cnt = nullptr;
  double* w = nullptr;
  double* z = nullptr;
};
size_t idx_bytes(uint64_t ns) { return sizeof(psg::FtrlmSlot) * ns; }
size_t cnt_bytes(uint64_t ns) { return 16 * (ns / 2 + 1); }
size_t row_bytes(uint64_t ns, int m) { return 8 * (size_t)m * (ns / 2 + 1); }

void store_put(psg_ctx* c, const Store& S, uint64_t ns, int m) {
  c->dev_put(S.idx, idx_bytes(ns));
  c->dev_put(S.cnt, cnt_bytes(ns));
  c->dev_put(S.w, row_bytes(ns, m));
  c->dev_put(S.z, row_bytes(ns, m));
}

// A store for ns slots on the context's stream: the index zeroed, the rows
// from `keep` on zeroed (the rows below it are the caller's to fill).
int store_get(psg_ctx* c, uint64_t ns, int m, uint64_t keep, Store* S) {
  int rc = c->dev_get(idx_bytes(ns), (void**)&S->idx, c->stream);
  if (rc == PSG_OK) rc = c->dev_get(cnt_bytes(ns), (void**)&S->cnt, c->stream);
  if (rc == PSG_OK) rc = c->dev_get(row_bytes(ns, m), (void**)&S->w, c->stream);
  if (rc == PSG_OK) rc = c->dev_get(row_bytes(ns, m), (void**)&S->z, c->stream);
  const size_t kc = 16 * keep, kr = 8 * (size_t)m * keep;
  if (rc == PSG_OK &&
      (hipMemsetAsync(S->idx, 0, idx_bytes(ns), c->stream) != hipSuccess ||
       hipMemsetAsync((char*)S->cnt + kc, 0, cnt_bytes(ns) - kc, c->stream) != hipSuccess ||
       hipMemsetAsync((char*)S->w + kr, 0, row_bytes(ns, m) - kr, c->stream) != hipSuccess ||
       hipMemsetAsync((char*)S->z + kr, 0, row_bytes(ns, m) - kr, c->stream) != hipSuccess))
    rc = fail(PSG_ERR_DEVICE, "multi-model FTRL: clearing the store");
  if (rc != PSG_OK) store_put(c, *S, ns, m);
  return rc;
}

// Growth to ns slots, on the context's stream and in the model's call order,
// no host wait: the index is rebuilt, the row store copied as it is.
int ftrlm_grow(psg_ctx* c, Ftrlm* F, uint64_t ns) {
  if (int rc = ftrlm_order(F, c->stream)) return rc;
  const uint64_t old_rows = F->row_cap();
  Store S;
  if (int rc = store_get(c, ns, F->m, old_rows, &S)) return rc;
  const psg::FtrlmTable from = F->table();
  psg::FtrlmTable to = from;
  to.idx = S.idx;
  to.mask = ns - 1;
  to.row_cap = ns / 2 + 1;
  const size_t rb = 8 * (size_t)F->m * old_rows;
  hipError_t e = psg::launch_ftrlm_rehash(from, to, c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(S.cnt, F->d_cnt, 16 * old_rows, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(S.w, F->d_w, rb, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(S.z, F->d_z, rb, hipMemcpyDeviceToDevice, c->stream);
  if (e != hipSuccess) {
    store_put(c, S, ns, F->m);
    return fail(PSG_ERR_DEVICE, "multi-model FTRL growth: %s", hipGetErrorString(e));
  }
  store_put(c, Store{F->d_idx, F->d_cnt, F->d_w, F->d_z}, F->nslots, F->m);
  F->d_idx = S.idx;
  F->d_cnt = S.cnt;
  F->d_w = S.w;
  F->d_z = S.z;
  F->nslots = ns;
  return ftrlm_mark(c, F, c->stream);
}

// pinned host words of this model: c->h_small[24 .. 31]
constexpr int kWords = 24;

// Room for n more keys: as ftrl_room.  The true entry count (rows handed out
// plus key 0) is read from the device only when the bound would pass the limit.
int ftrlm_room(psg_ctx* c, Ftrlm* F, size_t n) {
  if (F->bound + n > F->limit()) {
    if (int rc = ftrlm_order(F, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_small + kWords, F->d_head, 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    F->bound = (size_t)(c->h_small[kWords + 4] + (c->h_small[kWords + 3] ? 1 : 0));
    if (F->bound + n > F->limit()) {
      const uint64_t ns = std::max(2 * F->nslots, Ftrlm::slots_for(F->bound + n));
      if (int rc = ftrlm_grow(c, F, ns)) return rc;
    }
  }
  F->bound += n;
  return PSG_OK;
}

int ftrlm_report(psg_ctx* c, Ftrlm* F, unsigned long long rejected) {
  if (!rejected) return PSG_OK;
  HIP_TRY(hipMemsetAsync(&F->d_head->err, 0, 8, c->stream));
  if (int rc = ftrlm_mark(c, F, c->stream)) return rc;
  return fail(PSG_ERR_UNSORTED, "%llu key pairs of multi-model FTRL pushes not strictly "
              "increasing: those messages were not applied", rejected);
}

// a push into an evaluation-only model (psg_ftrlm_import_weights)
int ftrlm_unfrozen(Ftrlm* F) {
  if (F->frozen)
    return fail(PSG_ERR_ARG, "the multi-model FTRL is frozen: it was loaded by a weights-only "
                "import (evaluation only), z is unknown and a push would recompute w from it");
  return PSG_OK;
}

// The pinned host words of a state export: OR, AND, count, err.  They are
// psg_ctx_ftrl.hip's of the scalar export: either call reads them before it
// returns, under the context's lock.
constexpr int kStateWords = 20;

// Step 1 of a state export on stream s: *blk (state_count_bytes) holds the
// three device words and, from byte 64, the scan's tile sums; the host then
// knows the count, the key bits that differ and the rejected messages.  Waits.
size_t ftrlm_state_count_bytes(Ftrlm* F) { return 64 + 4 * psg::ftrlm_state_count_words(F->table()); }
int ftrlm_state_count(psg_ctx* c, Ftrlm* F, uint64_t lo, uint64_t hi, hipStream_t s, char** blk,
                size_t* n, uint64_t* differ, unsigned long long* rejected) {
  if (int rc = ftrlm_order(F, s)) return rc;
  if (int rc = c->dev_get(ftrlm_state_count_bytes(F), (void**)blk, s)) return rc;
  unsigned long long* small = (unsigned long long*)*blk;
  unsigned long long* h = c->h_small + kStateWords;
  if (int rc = psg::launch_ftrlm_state_count(F->table(), lo, hi, (uint32_t*)(*blk + 64), small, s))
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
void ftrlm_state_put(psg_ctx* c, Ftrlm* F, hipStream_t s, void* blk, size_t bytes) {
  if (!blk) return;
  if (s != c->stream && F->last) (void)hipStreamWaitEvent(c->stream, F->last, 0);
  c->dev_put(blk, bytes);
}

// Step 2: the n entries of [lo, hi] sorted by key into device arrays.
int ftrlm_state_emit(psg_ctx* c, Ftrlm* F, uint64_t lo, uint64_t hi, size_t n, uint64_t differ,
               const char* count_blk, uint64_t* keys, uint64_t* pos, uint64_t* neg, double* w,
               double* z, hipStream_t s) {
  if (n == 0) return PSG_OK;
  const size_t wb = psg::ftrlm_state_work_bytes(n);
  void* work = nullptr;
  if (int rc = c->dev_get(wb, &work, s)) return rc;
  int rc = psg::launch_ftrlm_state(F->table(), lo, hi, n, differ,
                                   (const uint32_t*)(count_blk + 64), work, keys, pos, neg, w, z, s);
  const int rm = ftrlm_mark(c, F, s);
  ftrlm_state_put(c, F, s, work, wb);
  return rc ? rc : rm;
}

int ftrlm_state_range(const uint64_t* range, uint64_t* lo, uint64_t* hi) {
  *lo = range ? range[0] : 0;
  *hi = range ? range[1] : ~0ull;
  if (*lo > *hi) return fail(PSG_ERR_ARG, "multi-model FTRL state export: range[0] > range[1]");
  return PSG_OK;
}

}  // namespace

int psg_ftrlm_init(psg_ctx* c, const psg_ftrl_param* p, int m, size_t capacity_hint) {
  if (!c || !p) return fail(PSG_ERR_ARG, "null argument");
  if (m < 1 || m > PSG_FTRL_MAX_MODELS)
    return fail(PSG_ERR_ARG, "%d models: 1 .. %d", m, PSG_FTRL_MAX_MODELS);
  std::lock_guard<std::mutex> l(c->mu);
  if (c->dtype != PSG_F64) return fail(PSG_ERR_ARG, "FTRL needs a PSG_F64 context");
  if (int rc = set_dev(c->device)) return rc;
  ftrlm_release(c);
  Ftrlm& F = c->ftrlm;
  const uint64_t ns = Ftrlm::slots_for(capacity_hint ? capacity_hint : (size_t(1) << 20));
  Store S;
  if (int rc = store_get(c, ns, m, 0, &S)) return rc;
  F.d_idx = S.idx;
  F.d_cnt = S.cnt;
  F.d_w = S.w;
  F.d_z = S.z;
  F.nslots = ns;
  F.m = m;
  psg::FtrlParam P[PSG_FTRL_MAX_MODELS] = {};
  for (int j = 0; j < m; ++j) P[j] = psg::FtrlParam{p[j].alpha, p[j].beta, p[j].lambda1, p[j].lambda2};
  int rc = c->dev_get(sizeof(psg::FtrlmHead), (void**)&F.d_head, c->stream);
  if (rc == PSG_OK &&
      (hipMemsetAsync(F.d_head, 0, sizeof(psg::FtrlmHead), c->stream) != hipSuccess ||
       hipMemcpyAsync(F.d_head->P, P, sizeof P, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
       hipStreamSynchronize(c->stream) != hipSuccess))  // P is this frame's
    rc = fail(PSG_ERR_DEVICE, "multi-model FTRL init");
  if (rc != PSG_OK) {
    ftrlm_release(c);
    return rc;
  }
  F.on = true;
  return ftrlm_mark(c, &F, c->stream);
}

int psg_ftrlm_reserve(psg_ctx* c, size_t entries) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (entries <= F->limit()) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  return ftrlm_grow(c, F, Ftrlm::slots_for(entries));
}

int psg_ftrlm_push_dev(psg_ctx* c, const uint64_t* keys, size_t n, const uint32_t* pos,
                       const uint32_t* neg, const double* grad, void* stream) {
  if (!c || (n && (!keys || !pos || !neg || !grad))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (int rc = ftrlm_unfrozen(F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrlm_room(c, F, n)) return rc;
  if (int rc = ftrlm_order(F, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_ftrlm_push(F->table(), keys, pos, neg, grad, n, (hipStream_t)stream));
  return ftrlm_mark(c, F, (hipStream_t)stream);
}

int psg_ftrlm_push(psg_ctx* c, const uint64_t* keys, size_t n, const uint32_t* pos,
                   const uint32_t* neg, const double* grad) {
  if (!c || (n && (!keys || !pos || !neg || !grad))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (int rc = ftrlm_unfrozen(F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrlm_room(c, F, n)) return rc;
  // one staging block for the four arrays, back to the pool after the kernels
  const size_t kb = align_up(8 * n, 256), gb = align_up(8 * n * F->m, 256),
               cb = align_up(4 * n, 256), b = kb + gb + 2 * cb;
  char* blk = nullptr;
  if (int rc = c->dev_get(b, (void**)&blk, c->copy)) return rc;
  int rc = c->h2d(blk, keys, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + kb, grad, 8 * n * F->m);
  if (rc == PSG_OK) rc = c->h2d(blk + kb + gb, pos, 4 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + kb + gb + cb, neg, 4 * n);
  if (rc == PSG_OK) rc = c->join_copy();
  if (rc == PSG_OK) rc = ftrlm_order(F, c->stream);
  if (rc == PSG_OK) {
    const hipError_t e = psg::launch_ftrlm_push(
        F->table(), (const uint64_t*)blk, (const uint32_t*)(blk + kb + gb),
        (const uint32_t*)(blk + kb + gb + cb), (const double*)(blk + kb), n, c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "ftrlm push: %s", hipGetErrorString(e));
  }
  if (rc == PSG_OK) rc = ftrlm_mark(c, F, c->stream);
  c->dev_put(blk, b);
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

int psg_ftrlm_pull_dev(psg_ctx* c, const uint64_t* keys, size_t n, double* out, void* stream) {
  if (!c || (n && (!keys || !out))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrlm_order(F, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_ftrlm_pull(F->table(), keys, n, out, (hipStream_t)stream));
  return ftrlm_mark(c, F, (hipStream_t)stream);
}

int psg_ftrlm_score_dev(psg_ctx* c, psg_minibatch* mb, int real, double* xw_dev, void* stream) {
  if (!c || !mb) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (int rc = set_dev(c->device)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (int rc = ftrlm_order(F, s)) return rc;
  const psg::FtrlmTable T = F->table();
  if (int rc = psg::mb_score(mb, c, nullptr, &T, real, xw_dev, s)) return rc;
  return ftrlm_mark(c, F, s);
}

int psg_ftrlm_pull(psg_ctx* c, const uint64_t* keys, size_t n, double* out) {
  if (!c || (n && (!keys || !out))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  const size_t kb = align_up(8 * n, 256), ob = 8 * n * F->m;
  if (int rc = c->ensure_scratch(kb + ob)) return rc;
  uint64_t* d_keys = (uint64_t*)c->scratch;
  double* d_out = (double*)((char*)c->scratch + kb);
  if (int rc = c->h2d(d_keys, keys, 8 * n)) return rc;
  if (int rc = c->join_copy()) return rc;
  if (int rc = ftrlm_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_ftrlm_pull(F->table(), d_keys, n, d_out, c->stream));
  if (int rc = ftrlm_mark(c, F, c->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small + kWords, F->d_head, 64, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (int rc = c->h2d_finish()) return rc;
  return ftrlm_report(c, F, c->h_small[kWords + 1]);
}

int psg_ftrlm_status(psg_ctx* c, size_t* entries, size_t* nnz, double* norm1, double* norm2) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrlm_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_ftrlm_status(F->table(), c->stream));
  if (int rc = ftrlm_mark(c, F, c->stream)) return rc;
  unsigned long long cnt[PSG_FTRL_MAX_MODELS];
  double norm[2 * PSG_FTRL_MAX_MODELS];
  HIP_TRY(hipMemcpyAsync(c->h_small + kWords, F->d_head, 64, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(cnt, F->d_head->nnz_res, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(norm, F->d_head->norm_res, sizeof norm, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const unsigned long long* h = c->h_small + kWords;
  if (h[2])  // unreachable while the load limit holds
    return fail(PSG_ERR_DEVICE, "multi-model FTRL table full: %llu keys were dropped", h[2]);
  F->bound = (size_t)(h[4] + (h[3] ? 1 : 0));
  if (entries) *entries = F->bound;
  for (int j = 0; j < F->m; ++j) {
    if (nnz) nnz[j] = (size_t)cnt[j];
    if (norm1) norm1[j] = norm[2 * j];
    if (norm2) norm2[j] = norm[2 * j + 1];
  }
  return ftrlm_report(c, F, h[1]);
}

int psg_ftrlm_export(psg_ctx* c, int j, uint64_t* keys, double* w, size_t cap, size_t* n) {
  if (!c || !n || (cap && (!keys || !w))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (j < 0 || j >= F->m) return fail(PSG_ERR_ARG, "model %d of %d", j, F->m);
  if (int rc = set_dev(c->device)) return rc;
  *n = 0;
  // model j's nonzero weights are counted first (the counter slots' sum): the
  // caller's room is checked and the scratch sized by that count
  if (int rc = ftrlm_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_ftrlm_count(F->table(), c->stream));
  if (int rc = ftrlm_mark(c, F, c->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(c->h_small + kWords, F->d_head, 64, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small + kWords + 6, &F->d_head->nnz_res[j], 8,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const unsigned long long rejected = c->h_small[kWords + 1];
  const size_t need = (size_t)c->h_small[kWords + 6];
  *n = need;
  if (need > cap)
    return fail(PSG_ERR_SIZE, "FTRL export: %zu nonzero weights, room for %zu", need, cap);
  if (need) {
    const size_t kb = align_up(8 * need, 256);
    if (int rc = c->ensure_scratch(2 * kb)) return rc;
    uint64_t* d_keys = (uint64_t*)c->scratch;
    double* d_w = (double*)((char*)c->scratch + kb);
    HIP_TRY(psg::launch_ftrlm_export(F->table(), j, d_keys, d_w, need, c->stream));
    if (int rc = ftrlm_mark(c, F, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(keys, d_keys, 8 * need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(w, d_w, 8 * need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return ftrlm_report(c, F, rejected);
}

int psg_ftrlm_import_dev(psg_ctx* c, const uint64_t* keys, size_t n, const uint64_t* pos,
                         const uint64_t* neg, const double* w, const double* z, void* stream) {
  if (!c || !keys || !pos || !neg || !w || !z)
    return fail(PSG_ERR_ARG, "multi-model FTRL import: keys, pos, neg, w and z are all required");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrlm_room(c, F, n)) return rc;
  if (int rc = ftrlm_order(F, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_ftrlm_import(F->table(), keys, pos, neg, w, z, n, (hipStream_t)stream));
  return ftrlm_mark(c, F, (hipStream_t)stream);
}

int psg_ftrlm_import(psg_ctx* c, const uint64_t* keys, size_t n, const uint64_t* pos,
                     const uint64_t* neg, const double* w, const double* z) {
  if (!c || !keys || !pos || !neg || !w || !z)
    return fail(PSG_ERR_ARG, "multi-model FTRL import: keys, pos, neg, w and z are all required");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrlm_room(c, F, n)) return rc;
  // one staging block for the five arrays, back to the pool after the kernels
  const size_t kb = align_up(8 * n, 256), rb = align_up(8 * n * F->m, 256), b = 3 * kb + 2 * rb;
  char* blk = nullptr;
  if (int rc = c->dev_get(b, (void**)&blk, c->copy)) return rc;
  int rc = c->h2d(blk, keys, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + kb, pos, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + 2 * kb, neg, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + 3 * kb, w, 8 * n * F->m);
  if (rc == PSG_OK) rc = c->h2d(blk + 3 * kb + rb, z, 8 * n * F->m);
  if (rc == PSG_OK) rc = c->join_copy();
  if (rc == PSG_OK) rc = ftrlm_order(F, c->stream);
  if (rc == PSG_OK) {
    const hipError_t e = psg::launch_ftrlm_import(
        F->table(), (const uint64_t*)blk, (const uint64_t*)(blk + kb),
        (const uint64_t*)(blk + 2 * kb), (const double*)(blk + 3 * kb),
        (const double*)(blk + 3 * kb + rb), n, c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "ftrlm import: %s", hipGetErrorString(e));
  }
  if (rc == PSG_OK) rc = ftrlm_mark(c, F, c->stream);
  c->dev_put(blk, b);
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

int psg_ftrlm_import_weights_dev(psg_ctx* c, int j, const uint64_t* keys, size_t n,
                                 const double* w, void* stream) {
  if (!c || (n && (!keys || !w))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (j < 0 || j >= F->m) return fail(PSG_ERR_ARG, "model %d of %d", j, F->m);
  if (n == 0) {  // an empty model file still freezes
    F->frozen = true;
    return PSG_OK;
  }
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrlm_room(c, F, n)) return rc;
  if (int rc = ftrlm_order(F, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_ftrlm_import_weights(F->table(), j, keys, w, n, (hipStream_t)stream));
  F->frozen = true;
  return ftrlm_mark(c, F, (hipStream_t)stream);
}

int psg_ftrlm_import_weights(psg_ctx* c, int j, const uint64_t* keys, size_t n, const double* w) {
  if (!c || (n && (!keys || !w))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (j < 0 || j >= F->m) return fail(PSG_ERR_ARG, "model %d of %d", j, F->m);
  if (n == 0) {  // an empty model file still freezes
    F->frozen = true;
    return PSG_OK;
  }
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = ftrlm_room(c, F, n)) return rc;
  const size_t kb = align_up(8 * n, 256), b = 2 * kb;
  char* blk = nullptr;
  if (int rc = c->dev_get(b, (void**)&blk, c->copy)) return rc;
  int rc = c->h2d(blk, keys, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(blk + kb, w, 8 * n);
  if (rc == PSG_OK) rc = c->join_copy();
  if (rc == PSG_OK) rc = ftrlm_order(F, c->stream);
  if (rc == PSG_OK) {
    const hipError_t e = psg::launch_ftrlm_import_weights(
        F->table(), j, (const uint64_t*)blk, (const double*)(blk + kb), n, c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "ftrlm import: %s", hipGetErrorString(e));
  }
  if (rc == PSG_OK) F->frozen = true;
  if (rc == PSG_OK) rc = ftrlm_mark(c, F, c->stream);
  c->dev_put(blk, b);
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

int psg_ftrlm_frozen(psg_ctx* c, int* frozen) {
  if (!c || !frozen) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  *frozen = F->frozen ? 1 : 0;
  return PSG_OK;
}

int psg_ftrlm_export_state_dev(psg_ctx* c, const uint64_t* range, uint64_t* keys, uint64_t* pos,
                               uint64_t* neg, double* w, double* z, size_t cap,
                               unsigned long long* n_dev, void* stream) {
  if (!c || !n_dev) return fail(PSG_ERR_ARG, "null argument");
  uint64_t lo, hi;
  if (int rc = ftrlm_state_range(range, &lo, &hi)) return rc;
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (int rc = set_dev(c->device)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char* cb = nullptr;
  const size_t cbytes = ftrlm_state_count_bytes(F);
  size_t n = 0;
  uint64_t differ = 0;
  unsigned long long rejected = 0;
  int rc = ftrlm_state_count(c, F, lo, hi, s, &cb, &n, &differ, &rejected);
  if (rc == PSG_OK && hipMemcpyAsync(n_dev, cb + 16, 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
    rc = fail(PSG_ERR_DEVICE, "ftrlm state export: count copy");
  if (rc == PSG_OK && n > cap)
    rc = fail(PSG_ERR_SIZE, "multi-model FTRL state export: %zu entries, room for %zu", n, cap);
  else if (rc == PSG_OK)
    rc = ftrlm_state_emit(c, F, lo, hi, n, differ, cb, keys, pos, neg, w, z, s);
  const int rm = ftrlm_mark(c, F, s);
  ftrlm_state_put(c, F, s, cb, cbytes);
  if (rc != PSG_OK || rm != PSG_OK) return rc ? rc : rm;
  return ftrlm_report(c, F, rejected);
}

int psg_ftrlm_export_state(psg_ctx* c, const uint64_t* range, uint64_t* keys, uint64_t* pos,
                           uint64_t* neg, double* w, double* z, size_t cap, size_t* n_out) {
  if (!c || !n_out) return fail(PSG_ERR_ARG, "null argument");
  uint64_t lo, hi;
  if (int rc = ftrlm_state_range(range, &lo, &hi)) return rc;
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (int rc = set_dev(c->device)) return rc;
  *n_out = 0;
  hipStream_t s = c->stream;
  char* cb = nullptr;
  const size_t cbytes = ftrlm_state_count_bytes(F);
  size_t n = 0;
  uint64_t differ = 0;
  unsigned long long rejected = 0;
  int rc = ftrlm_state_count(c, F, lo, hi, s, &cb, &n, &differ, &rejected);
  if (rc == PSG_OK) *n_out = n;
  if (rc == PSG_OK && n > cap)
    rc = fail(PSG_ERR_SIZE, "multi-model FTRL state export: %zu entries, room for %zu", n, cap);
  void* const dst[5] = {keys, pos, neg, w, z};
  const bool any = keys || pos || neg || w || z;
  if (rc == PSG_OK && n && any) {
    // keys, pos, neg of 8 n bytes, then the w and z rows of 8 n m bytes
    const size_t kb = align_up(8 * n, 256), rb = align_up(8 * n * F->m, 256);
    const size_t off[5] = {0, kb, 2 * kb, 3 * kb, 3 * kb + rb};
    const size_t len[5] = {8 * n, 8 * n, 8 * n, 8 * n * F->m, 8 * n * F->m};
    char* ob = nullptr;
    rc = c->dev_get(3 * kb + 2 * rb, (void**)&ob, s);
    if (rc == PSG_OK) {
      void* d[5];
      for (int i = 0; i < 5; ++i) d[i] = dst[i] ? ob + off[i] : nullptr;
      rc = ftrlm_state_emit(c, F, lo, hi, n, differ, cb, (uint64_t*)d[0], (uint64_t*)d[1],
                      (uint64_t*)d[2], (double*)d[3], (double*)d[4], s);
      for (int i = 0; i < 5 && rc == PSG_OK; ++i)
        if (dst[i] &&
            hipMemcpyAsync(dst[i], d[i], len[i], hipMemcpyDeviceToHost, s) != hipSuccess)
          rc = fail(PSG_ERR_DEVICE, "ftrlm state export: copy to the host");
      if (hipStreamSynchronize(s) != hipSuccess && rc == PSG_OK)
        rc = fail(PSG_ERR_DEVICE, "ftrlm state export: wait");
      c->dev_put(ob, 3 * kb + 2 * rb);
    }
  }
  c->dev_put(cb, cbytes);
  if (rc != PSG_OK) return rc;
  return ftrlm_report(c, F, rejected);
}

int psg_ftrlm_lookup(psg_ctx* c, const uint64_t* keys, size_t n, uint64_t* pos, uint64_t* neg,
                     double* w, double* z, uint8_t* found) {
  if (!c || (n && !keys)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Ftrlm* F;
  if (int rc = ftrlm_of(c, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  const size_t kb = align_up(8 * n, 256), rb = align_up(8 * n * F->m, 256);
  if (int rc = c->ensure_scratch(4 * kb + 2 * rb)) return rc;
  char* s = (char*)c->scratch;
  char* const at[5] = {s + kb, s + 2 * kb, s + 3 * kb, s + 3 * kb + rb, s + 3 * kb + 2 * rb};
  if (int rc = c->h2d(s, keys, 8 * n)) return rc;
  if (int rc = c->join_copy()) return rc;
  if (int rc = ftrlm_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_ftrlm_lookup(F->table(), (const uint64_t*)s, n, (uint64_t*)at[0],
                                   (uint64_t*)at[1], (double*)at[2], (double*)at[3],
                                   (uint8_t*)at[4], c->stream));
  if (int rc = ftrlm_mark(c, F, c->stream)) return rc;
  void* const dst[5] = {pos, neg, w, z, found};
  const size_t len[5] = {8 * n, 8 * n, 8 * n * F->m, 8 * n * F->m, n};
  for (int i = 0; i < 5; ++i)
    if (dst[i]) HIP_TRY(hipMemcpyAsync(dst[i], at[i], len[i], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return c->h2d_finish();
}

}  // extern "C"

void psg::ftrlm_release(psg_ctx* c) {
  Ftrlm& F = c->ftrlm;
  if (F.last) {
    (void)hipEventSynchronize(F.last);
    c->free_ev.push_back(F.last);
    F.last = nullptr;
  }
  if (F.nslots) {
    c->dev_put(F.d_idx, sizeof(psg::FtrlmSlot) * F.nslots);
    c->dev_put(F.d_cnt, 16 * (F.nslots / 2 + 1));
    c->dev_put(F.d_w, 8 * (size_t)F.m * (F.nslots / 2 + 1));
    c->dev_put(F.d_z, 8 * (size_t)F.m * (F.nslots / 2 + 1));
  }
  c->dev_put(F.d_head, sizeof(psg::FtrlmHead));
  F = Ftrlm();
}
