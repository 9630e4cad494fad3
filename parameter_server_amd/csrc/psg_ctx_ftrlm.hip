// psg_ctx_ftrlm.hip -- the multi-model FTRL of a context (psg_ftrlm_*,
// include/psg.h) over the kernels of psg_ftrl_rows.hip.  The contract is
// psg_ctx_ftrl.hip's: messages apply in call order whatever the stream, a push
// allocates nothing and waits for nothing while the model has room, and a
// rejected message is reported once by the next call that synchronises.
#include "psg_ctx.h"

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
