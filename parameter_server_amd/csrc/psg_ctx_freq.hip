// psg_ctx_freq.hip -- the frequency filter of a context's channels
// (FreqencyFilter<uint64>: psg_freq_*, include/psg.h) over the count-min
// kernels of psg_countmin.hip.
#include "psg_ctx.h"

extern "C" {

// ------------------------------------------------------ frequency filter --
namespace {
int filter_order(Filter* F, hipStream_t s);
int filter_mark(psg_ctx* c, Filter* F, hipStream_t s);
}  // namespace

int psg_freq_resize(psg_ctx* c, int chl, int n, int k) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  if (int rc = set_dev(c->device)) return rc;
  Filter& F = c->ff[chl];
  const uint32_t nn = (uint32_t)std::max(n, 64);  // countmin.h:15
  F.sync_ext();
  if (nn != F.n) {
    c->dev_put(F.d_table, psg::cm_table_bytes(F.n));
    F.d_table = nullptr;
    F.n = 0;
    if (int rc = c->dev_get(psg::cm_table_bytes(nn), (void**)&F.d_table, c->stream)) return rc;
    F.n = nn;
  }
  F.k = std::min(30, std::max(1, k));  // countmin.h:18
  // the clear joins the filter's call order: after the filter's
  // previous operation on any stream, and before the next one on any stream
  // (a caller stream, the null stream included, does not wait for the
  // non-blocking context stream by itself)
  if (int rc = filter_order(&F, c->stream)) return rc;
  HIP_TRY(hipMemsetAsync(F.d_table, 0, psg::cm_table_bytes(F.n), c->stream));
  return filter_mark(c, &F, c->stream);
}

int psg_freq_clear(psg_ctx* c, int chl) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ff.find(chl);
  if (it != c->ff.end()) {
    filter_release(c, it->second);
    c->ff.erase(it);
  }
  return PSG_OK;
}

int psg_freq_empty(psg_ctx* c, int chl, int* empty) {
  if (!c || !empty) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ff.find(chl);
  *empty = it == c->ff.end() || it->second.n == 0;
  return PSG_OK;
}

namespace {
int filter_of(psg_ctx* c, int chl, Filter** F) {
  auto it = c->ff.find(chl);
  if (it == c->ff.end() || it->second.n == 0)
    return fail(PSG_ERR_ARG, "channel %d: frequency filter is empty (psg_freq_resize)", chl);
  *F = &it->second;
  return PSG_OK;
}

// the binned insert's scratch for n keys (stream s: where the insert runs);
// a filter too large to bin gets none (the CAS form runs)
int filter_bins(psg_ctx* c, Filter* F, size_t n, hipStream_t s) {
  const size_t need = psg::cm_insert_scratch_bytes(n, F->n, F->k);
  if (need == 0 || need <= F->bins_bytes) return PSG_OK;
  F->sync_ext();
  c->dev_put(F->d_bins, F->bins_bytes);
  F->d_bins = nullptr;
  F->bins_bytes = 0;
  if (int rc = c->dev_get(need, &F->d_bins, s)) return rc;
  F->bins_bytes = need;
  return PSG_OK;
}

// order an operation on stream s after the filter's previous one
int filter_order(Filter* F, hipStream_t s) {
  if (F->last && F->last_s != s) HIP_TRY(hipStreamWaitEvent(s, F->last, 0));
  return PSG_OK;
}
// ... and mark it as the filter's last
int filter_mark(psg_ctx* c, Filter* F, hipStream_t s) {
  if (!F->last)
    if (int rc = c->event(&F->last)) return rc;
  HIP_TRY(hipEventRecord(F->last, s));
  F->last_s = s;
  return PSG_OK;
}
}  // namespace

int psg_freq_insert_dev(psg_ctx* c, int chl, const uint64_t* keys, const uint32_t* counts,
                        size_t n, void* stream) {
  if (!c || (n && (!keys || !counts))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Filter* F;
  if (int rc = filter_of(c, chl, &F)) return rc;
  if (int rc = filter_order(F, (hipStream_t)stream)) return rc;
  if (int rc = filter_bins(c, F, n, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_cm_insert(keys, counts, n, F->d_table, F->n, F->k, F->d_bins,
                                F->bins_bytes, (hipStream_t)stream));
  F->ext = (hipStream_t)stream;
  F->ext_used = true;
  return filter_mark(c, F, (hipStream_t)stream);
}

size_t psg_freq_query_scratch_bytes(size_t n) { return psg::cm_query_scratch_bytes(n); }

int psg_freq_query_dev(psg_ctx* c, int chl, const uint64_t* keys, size_t n, int freq,
                       uint64_t* out, unsigned long long* nout, void* scratch, void* stream) {
  if (!c || !nout || !scratch || (n && (!keys || !out))) return fail(PSG_ERR_ARG, "null argument");
  if (freq >= 255) return fail(PSG_ERR_ARG, "freqency %d >= kuint8max", freq);  // :29
  std::lock_guard<std::mutex> l(c->mu);
  Filter* F;
  if (int rc = filter_of(c, chl, &F)) return rc;
  if (int rc = filter_order(F, (hipStream_t)stream)) return rc;
  HIP_TRY(psg::launch_cm_query(keys, n, F->d_table, F->n, F->k, freq, out, nout, scratch,
                               (hipStream_t)stream));
  F->ext = (hipStream_t)stream;
  F->ext_used = true;
  return filter_mark(c, F, (hipStream_t)stream);
}

int psg_freq_insert(psg_ctx* c, int chl, const uint64_t* keys, const uint32_t* counts,
                    size_t n) {
  if (!c || (n && (!keys || !counts))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Filter* F;
  if (int rc = filter_of(c, chl, &F)) return rc;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  // one staging block for keys + counts, back to the pool after the kernel
  const size_t kb = align_up(8 * n, 256), b = kb + 4 * n;
  void* blk = nullptr;
  if (int rc = c->dev_get(b, &blk, c->copy)) return rc;
  int rc = c->h2d(blk, keys, 8 * n);
  if (rc == PSG_OK) rc = c->h2d((char*)blk + kb, counts, 4 * n);
  if (rc == PSG_OK) rc = c->join_copy();
  if (rc == PSG_OK) rc = filter_order(F, c->stream);
  if (rc == PSG_OK) rc = filter_bins(c, F, n, c->stream);
  if (rc == PSG_OK) {
    hipError_t e = psg::launch_cm_insert((const uint64_t*)blk, (const uint32_t*)((char*)blk + kb),
                                         n, F->d_table, F->n, F->k, F->d_bins, F->bins_bytes,
                                         c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "freq insert: %s", hipGetErrorString(e));
  }
  if (rc == PSG_OK) rc = filter_mark(c, F, c->stream);
  c->dev_put(blk, b);
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

int psg_freq_query(psg_ctx* c, int chl, const uint64_t* keys, size_t n, int freq, uint64_t* out,
                   size_t* nout) {
  if (!c || !nout || (n && (!keys || !out))) return fail(PSG_ERR_ARG, "null argument");
  if (freq >= 255) return fail(PSG_ERR_ARG, "freqency %d >= kuint8max", freq);
  std::lock_guard<std::mutex> l(c->mu);
  Filter* F;
  if (int rc = filter_of(c, chl, &F)) return rc;
  *nout = 0;
  if (n == 0) return PSG_OK;
  if (int rc = set_dev(c->device)) return rc;
  const size_t kb = align_up(8 * n, 256), sb = psg::cm_query_scratch_bytes(n);
  if (int rc = c->ensure_scratch(2 * kb + sb)) return rc;
  uint64_t* d_keys = (uint64_t*)c->scratch;
  uint64_t* d_out = (uint64_t*)((char*)c->scratch + kb);
  void* d_s = (char*)c->scratch + 2 * kb;
  if (int rc = c->h2d(d_keys, keys, 8 * n)) return rc;
  if (int rc = c->join_copy()) return rc;
  if (int rc = filter_order(F, c->stream)) return rc;
  HIP_TRY(psg::launch_cm_query(d_keys, n, F->d_table, F->n, F->k, freq, d_out, c->d_small + 7,
                               d_s, c->stream));
  if (int rc = filter_mark(c, F, c->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(c->h_small + 7, c->d_small + 7, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t m = (size_t)c->h_small[7];
  if (m) HIP_TRY(hipMemcpy(out, d_out, 8 * m, hipMemcpyDeviceToHost));
  *nout = m;
  return c->h2d_finish();
}

int psg_freq_table(psg_ctx* c, int chl, uint8_t* out, size_t n) {
  if (!c || (n && !out)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Filter* F;
  if (int rc = filter_of(c, chl, &F)) return rc;
  if (n > F->n) return fail(PSG_ERR_ARG, "table copy of %zu > %u counters", n, F->n);
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = filter_order(F, c->stream)) return rc;
  if (n) HIP_TRY(hipMemcpyAsync(out, F->d_table, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PSG_OK;
}

int psg_freq_table_assign(psg_ctx* c, int chl, const uint8_t* table, size_t n) {
  if (!c || (n && !table)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  Filter* F;
  if (int rc = filter_of(c, chl, &F)) return rc;
  if (n != F->n) return fail(PSG_ERR_SIZE, "table of %zu counters for a filter of %u", n, F->n);
  if (int rc = set_dev(c->device)) return rc;
  // in the filter's call order; the caller's array is free on return
  if (int rc = filter_order(F, c->stream)) return rc;
  HIP_TRY(hipMemcpyAsync(F->d_table, table, n, hipMemcpyHostToDevice, c->stream));
  if (int rc = filter_mark(c, F, c->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PSG_OK;
}

}  // extern "C"

void psg::filter_release(psg_ctx* c, Filter& F) {
  F.sync_ext();
  if (F.last) {
    (void)hipEventSynchronize(F.last);
    c->free_ev.push_back(F.last);
    F.last = nullptr;
  }
  c->dev_put(F.d_table, psg::cm_table_bytes(F.n));
  c->dev_put(F.d_bins, F.bins_bytes);
  F.d_table = nullptr;
  F.d_bins = nullptr;
}
