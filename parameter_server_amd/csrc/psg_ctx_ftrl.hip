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
