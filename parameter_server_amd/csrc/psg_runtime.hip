// psg_runtime.hip -- host side of the C ABI (include/psg.h): the context
// core.  Create / destroy, the block pool and slabs (psg_ctx.h), keys and
// values, the push family, received, darling; and the last-error text.
#include "psg_ctx.h"

namespace {
thread_local std::string g_err;
// psg_push tests pushes of at least this many keys for a contiguous slice
constexpr size_t kDenseMinKeys = 1024;
}  // namespace

int psg::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

void psg::ctx_info(psg_ctx* c, int* device, int* dtype, hipStream_t* stream) {
  *device = c->device;
  *dtype = c->dtype;
  *stream = c->stream;
}

extern "C" {

int psg_abi_version(void) { return PSG_ABI_VERSION; }

const char* psg_status_string(int s) {
  switch (s) {
    case PSG_OK: return "ok";
    case PSG_ERR_ARG: return "invalid argument";
    case PSG_ERR_UNMATCHED: return "pushed key not matched";
    case PSG_ERR_RANGE: return "position range mismatch";
    case PSG_ERR_NO_TIME: return "no data received at time";
    case PSG_ERR_OOM: return "out of device memory";
    case PSG_ERR_DEVICE: return "device error";
    case PSG_ERR_UNSORTED: return "keys not strictly increasing";
    case PSG_ERR_SIZE: return "value/key size mismatch";
    case PSG_ERR_CHANNEL: return "channel mismatch";
    case PSG_ERR_EMPTY_KEYS: return "channel has no server keys";
    case PSG_ERR_SIGNATURE: return "key signature mismatch";
    default: return "unknown status";
  }
}

const char* psg_last_error(void) { return g_err.c_str(); }

int psg_device_count(int* n) {
  if (!n) return fail(PSG_ERR_ARG, "null");
  HIP_TRY(hipGetDeviceCount(n));
  return PSG_OK;
}

// --------------------------------------------------------------- context --
int psg_create(int device, int dtype, unsigned flags, psg_ctx** out) {
  if (!out) return fail(PSG_ERR_ARG, "null out");
  if (dtype != PSG_F32 && dtype != PSG_F64) return fail(PSG_ERR_ARG, "dtype %d", dtype);
  if (int rc = set_dev(device)) return rc;
  psg_ctx* c = new psg_ctx();
  c->device = device;
  c->dtype = dtype;
  c->flags = flags;
  c->table.read_knobs(flags);
  c->zero_copy = !(flags & PSG_NO_ZERO_COPY);
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->copy_ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&c->d_small, 256);
  // zeroed: the deferred-error words of the device forms (psg_ctx_dev.hip)
  if (e == hipSuccess) e = hipMemsetAsync(c->d_small, 0, 256, c->stream);
  if (e == hipSuccess) e = hipMalloc((void**)&c->d_vio_slots, 64 * psg::kVioSlots);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_vio_slots, 0, 64 * psg::kVioSlots, c->stream);
  if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_small, 256);
  if (e != hipSuccess) {
    psg_destroy(c);
    return fail(PSG_ERR_DEVICE, "psg_create: %s", hipGetErrorString(e));
  }
  *out = c;
  return PSG_OK;
}


int psg_destroy(psg_ctx* c) {
  if (!c) return PSG_OK;
  (void)hipSetDevice(c->device);
  c->zc.n = 0;  // held buffers of pushes never merged: not read any more
  if (c->copy) (void)hipStreamSynchronize(c->copy);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& kv : c->agg) c->drop(kv.second);
  c->agg.clear();
  c->kcache.clear();
  for (auto& kv : c->ch) {
    if (kv.second.last) {  // the device forms' last operation, on a caller's stream
      (void)hipEventSynchronize(kv.second.last);
      c->free_ev.push_back(kv.second.last);
    }
    c->dev_put(kv.second.d_dev, kChanWordBytes);
    c->dev_put(kv.second.d_keys, kv.second.kbytes);
    c->dev_put(kv.second.d_vals, kv.second.nvals * vsize(c->dtype));
    c->dev_put(kv.second.d_delta, 8 * kv.second.dn);
    c->dev_put(kv.second.d_active, 4 * ((kv.second.dn + 31) / 32));
    (void)kv.second.mirror();
    if (kv.second.hk) (void)hipHostFree(kv.second.hk);
    if (kv.second.hev) (void)hipEventDestroy(kv.second.hev);
  }
  c->ch.clear();
  for (auto& kv : c->ff) filter_release(c, kv.second);
  c->ff.clear();
  ftrl_release(c);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& f : c->fly) c->free_ev.push_back(f.ev);
  c->fly.clear();
  c->table.release();
  c->pool_release();
  c->ctr_release();
  if (c->ring) (void)hipHostFree(c->ring);
  (void)hipFree(c->d_small);
  (void)hipFree(c->d_vio_slots);
  if (c->h_small) (void)hipHostFree(c->h_small);
  (void)hipFree(c->scratch);
  if (c->copy_ev) (void)hipEventDestroy(c->copy_ev);
  if (c->done_ev) (void)hipEventDestroy(c->done_ev);
  if (c->copy) (void)hipStreamDestroy(c->copy);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return PSG_OK;
}

int psg_set_match_flags(psg_ctx* c, unsigned flags) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  if (c->zc.n) HIP_TRY(hipSetDevice(c->device));
  if (int rc = c->zc_flush()) return rc;  // held copies were queued under the old mode
  c->flags = flags;
  c->table.read_knobs(flags);
  c->zero_copy = !(flags & PSG_NO_ZERO_COPY);
  return PSG_OK;
}

int psg_set_flush_pushes(psg_ctx* c, int n) {
  if (!c || n < 1 || n > psg::kMaxPush) return fail(PSG_ERR_ARG, "flush pushes %d", n);
  std::lock_guard<std::mutex> l(c->mu);
  c->flush_pushes = (size_t)n;
  return PSG_OK;
}

namespace {

// The host mirror of a changed key set: one asynchronous device-to-host copy
// into pinned memory on `stream`, waited for by the first reader.
int refresh_mirror(psg_ctx* c, Channel& C) {
  (void)C.mirror();  // the previous copy may still target the buffer
  if (C.n > C.hcap) {
    if (C.hk) HIP_TRY(hipHostFree(C.hk));
    C.hk = nullptr;
    C.hcap = 0;
    const size_t cap = std::max(C.n, C.n + C.n / 2);
    HIP_TRY(hipHostMalloc((void**)&C.hk, 8 * cap));
    C.hcap = cap;
  }
  if (!C.hev) HIP_TRY(hipEventCreateWithFlags(&C.hev, hipEventDisableTiming));
  if (C.n) HIP_TRY(hipMemcpyAsync(C.hk, C.d_keys, 8 * C.n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(C.hev, c->stream));
  C.hpend = true;
  return PSG_OK;
}

// key_[chl] = key_[chl].setUnion(keys_0).setUnion(keys_1)...; val_[chl].clear()
// (kv_vector.h:177-182, shared_array_inl.h:155-162) for resident key-only
// pushes d_push[i] (n[i] keys): one N-way merge on the device (psg_nway.hip)
// of the server keys and up to 63 pushes at a time; the host mirror is then
// refreshed from the device result by an asynchronous copy (no CPU union).
int key_union_impl(psg_ctx* c, int chl, const std::vector<const uint64_t*>& d_push,
                   const std::vector<uint64_t>& n) {
  Channel& C = c->ch[chl];
  // Pending value pushes of this channel were matched against the current
  // key_[chl] in the reference (setValue matches at arrival,
  // kv_vector.h:171-204): enqueue their merge before the key set (and so
  // every position) changes.  The old key array goes back to the pool after
  // those kernels.
  for (auto& kv : c->agg)
    if (kv.second.chl == chl && !kv.second.pending.empty())
      if (int rc = c->flush(kv.second)) return rc;
  if (int rc = c->join_copy()) return rc;
  // ... and after the device pulls still reading the keys and values
  if (int rc = c->chan_order(C, c->stream)) return rc;
  bool changed = false;
  // once a merge applied, the key set (so every position) changed: the
  // mirror is refreshed and val_[chl] cleared (kv_vector.h:180) on every
  // way out, an error in a later chunk of pushes included
  auto settle = [&](int rc) -> int {
    if (!changed) return rc;
    const int mr = refresh_mirror(c, C);
    c->dev_put(C.d_vals, C.nvals * vsize(c->dtype));
    C.d_vals = nullptr;
    C.nvals = 0;
    return rc != PSG_OK ? rc : mr;
  };
  for (size_t i = 0; i < d_push.size();) {
    std::vector<const uint64_t*> pk;
    std::vector<uint64_t> pn;
    if (C.n) {
      pk.push_back(C.d_keys);
      pn.push_back(C.n);
    }
    const size_t base = pk.size();
    for (; i < d_push.size() && pk.size() < (size_t)psg_nway_max_push(); ++i)
      if (n[i]) {
        pk.push_back(d_push[i]);
        pn.push_back(n[i]);
      }
    if (pk.size() == base) continue;  // only empty pushes: ignored (kv_vector.h:177)
    uint64_t cap = 0;
    for (uint64_t x : pn) cap += x;
    if (cap >= (1ull << 32))
      return settle(fail(PSG_ERR_ARG, "key union of %llu keys >= 2^32", (unsigned long long)cap));
    const uint32_t K = (uint32_t)pk.size();
    if (int rc = c->ensure_scratch(psg::nway_scratch_bytes(K, pn.data()))) return settle(rc);
    uint64_t* d_out = nullptr;
    if (int rc = c->dev_get(8 * cap, (void**)&d_out, c->stream)) return settle(rc);
    unsigned long long* d_bad = nullptr;
    hipError_t e = psg::nway_union_enqueue(K, pk.data(), pn.data(), d_out, c->scratch, &d_bad,
                                           c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(c->h_small, d_bad, 16, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      c->dev_put(d_out, 8 * cap);
      return settle(fail(PSG_ERR_DEVICE, "key union: %s", hipGetErrorString(e)));
    }
    const unsigned long long bad = c->h_small[0], nu = c->h_small[1];
    if (bad) {  // the pushes of this merge are not applied; earlier ones are
      c->dev_put(d_out, 8 * cap);
      // high bits (tile overflow / look-back timeout): a device fault only
      // if every push is strictly increasing
      bool dis = false;
      if (bad >> 32) {
        e = psg::nway_disordered(K, pk.data(), pn.data(), c->stream, &dis);
        if (e != hipSuccess)
          return settle(fail(PSG_ERR_DEVICE, "key union: %s", hipGetErrorString(e)));
      }
      return settle(fail((bad >> 32) && !dis ? PSG_ERR_DEVICE : PSG_ERR_UNSORTED,
                         "key-only push: %llu order violations", bad));
    }
    c->dev_put(C.d_keys, C.kbytes);
    C.d_keys = d_out;
    C.kbytes = 8 * cap;
    C.n = (size_t)nu;
    changed = true;
  }
  return settle(PSG_OK);
}

}  // namespace

// findRange of a push and the consistency checks of setValue, before any
// data is staged
int psg_ctx::check_push(int chl, int time, uint64_t kb, uint64_t ke, size_t n, int m,
                        size_t* lo, size_t* hi) {
  psg_ctx* c = this;
  if (m < 1 || m > PSG_MAX_VALUE_ARRAYS) return fail(PSG_ERR_ARG, "m=%d", m);
  if (ke < kb) return fail(PSG_ERR_ARG, "invalid key range");
  auto cit = c->ch.find(chl);
  if (cit == c->ch.end() || cit->second.n == 0)
    return fail(PSG_ERR_EMPTY_KEYS, "channel %d has no server keys", chl);
  Channel& C = cit->second;
  const uint64_t* h = C.mirror();
  *lo = std::lower_bound(h, h + C.n, kb) - h;
  *hi = std::lower_bound(h, h + C.n, ke) - h;
  if (*hi - *lo < n)  // pigeonhole: some key cannot match (CHECK_GE, kv_vector.h:121,191)
    return fail(PSG_ERR_UNMATCHED, "push of %zu keys into a range of %zu server keys", n,
                *hi - *lo);
  auto ait = c->agg.find(time);
  if (ait != c->agg.end()) {
    const Aggregate& A = ait->second;
    if (A.chl != chl) return fail(PSG_ERR_CHANNEL, "time %d: channel %d != %d", time, chl, A.chl);
    if (A.lo != *lo || A.hi != *hi)  // CHECK_EQ(aligned.first, stored) kv_vector.h:199
      return fail(PSG_ERR_RANGE, "time %d: range [%zu,%zu) != [%zu,%zu)", time, *lo, *hi,
                  A.lo, A.hi);
  }
  return PSG_OK;
}

int psg_ctx::decode_pending(Aggregate& a, size_t take, void** blk, size_t* bytes) {
  *blk = nullptr;
  *bytes = 0;
  std::vector<uint64_t> pr, dst, cap;
  for (size_t p = 0; p < take; ++p) {
    PendingPush& pp = a.pending[p];
    for (int i = 0; i < pp.cparts; ++i) {
      pr.push_back(pp.cbeg[i]);
      pr.push_back(pp.cend[i]);
      dst.push_back(pp.cdst[i]);
      cap.push_back(pp.ccap[i]);
    }
    pp.cparts = 0;
  }
  const size_t n = dst.size();
  if (n == 0) return PSG_OK;
  // held pushes' parts may still sit in the zero-copy batch: issue it first
  if (int rc = zc_flush()) return rc;
  // [pairs 16n][dst 8n][cap 8n] | [status 4n] | decoder scratch
  const size_t hb = 32 * n, sb = align_up(hb + 4 * n, 256);
  const size_t total = sb + psg::snappy_scratch_bytes(n);
  void* b = nullptr;
  if (int rc = dev_get(total, &b, copy)) return rc;
  std::vector<uint64_t> img(4 * n);
  std::copy(pr.begin(), pr.end(), img.begin());
  std::copy(dst.begin(), dst.end(), img.begin() + 2 * n);
  std::copy(cap.begin(), cap.end(), img.begin() + 3 * n);
  int rc = h2d(b, img.data(), hb);
  if (rc == PSG_OK) {
    const uint64_t* d = (const uint64_t*)b;
    const hipError_t e = psg::launch_snappy(nullptr, d, n, nullptr, d + 2 * n, d + 3 * n,
                                            (int32_t*)(d + 4 * n), (char*)b + sb, copy,
                                            a.d_bad + 1, true);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "snappy: %s", hipGetErrorString(e));
  }
  if (rc != PSG_OK) {
    (void)hipStreamSynchronize(copy);
    dev_put(b, total);
    return rc;
  }
  *blk = b;
  *bytes = total;
  return PSG_OK;
}

int psg_ctx::aggregate_for(int chl, int time, uint64_t kb, uint64_t ke, int m,
                           Aggregate** out) {
  auto ait = agg.find(time);
  if (ait == agg.end()) {
    // (re-derived: the caller checked the push against the range)
    Channel& C = ch[chl];
    const uint64_t* h = C.mirror();
    const size_t lo = std::lower_bound(h, h + C.n, kb) - h;
    const size_t hi = std::lower_bound(h, h + C.n, ke) - h;
    Aggregate A;
    A.chl = chl;
    A.lo = lo;
    A.hi = hi;
    // zeroed on `copy`: the dense pushes' order checks and the compressed
    // pushes' decodes add to it there; every reader on `stream` runs after
    // a join_copy
    if (int rc = dev_get(kBadBytes, (void**)&A.d_bad, copy)) return rc;
    HIP_TRY(hipMemsetAsync(A.d_bad, 0, kBadBytes, copy));
    ait = agg.emplace(time, A).first;
  }
  Aggregate& A = ait->second;
  // a push with more value arrays than the earlier ones extends the list
  // (recved_val_[t].push_back, kv_vector.h:118-125,193-194)
  for (; A.m < m; ++A.m)
    if (int rc = dev_get((A.hi - A.lo) * vsize(dtype), &A.d_out[A.m], stream)) return rc;
  *out = &A;
  return PSG_OK;
}

int psg_ctx::push_values(int chl, int time, uint64_t kb, uint64_t ke, const KeyRef& keys, int m,
                         const void* const* vals, void* vblock, const size_t* slice,
                         void* sblock, size_t sbytes, const PendingPush* comp) {
  const size_t sv = vsize(dtype), n = keys->n;
  PendingPush pp;
  if (comp) pp = *comp;  // the compressed parts to decode
  pp.n = n;
  pp.m = m;
  pp.keys = keys;
  pp.sblock = sblock;
  pp.sbytes = sbytes;
  const size_t vb = align_up(sv * n, 256);
  pp.vbytes = m * vb;
  if (vblock) {
    pp.vblock = vblock;
    for (int i = 0; i < m; ++i) pp.d_vals[i] = (char*)pp.vblock + i * vb;
  } else {
    if (int rc = dev_get(pp.vbytes, &pp.vblock, copy)) return rc;
    for (int i = 0; i < m; ++i) {
      pp.d_vals[i] = (char*)pp.vblock + i * vb;
      if (int rc = h2d(pp.d_vals[i], vals[i], sv * n, true)) {
        release_push(pp);
        return rc;
      }
    }
  }
  Aggregate* Ap = nullptr;
  if (int rc = aggregate_for(chl, time, kb, ke, m, &Ap)) {
    release_push(pp);
    return rc;
  }
  Aggregate& A = *Ap;
  if (slice) {
    pp.dense = true;
    pp.dpos = *slice - A.lo;
    pp.kd = ch[chl].d_keys + *slice;
    if (keys->d) {
      HIP_TRY(psg::launch_check_sorted(keys->d, n, A.d_bad, copy, true));
    } else if (keys->host) {  // neither: a device push's claim, checked by its intake
      HIP_TRY(psg::launch_check_sorted_host(keys->host, n, A.d_bad, copy));
      pinned_wait = pinned_wait || !(flags & PSG_HOLD_BUFFERS);
    }
  }
  A.pending.push_back(pp);
  A.expected_total += n;
  if (A.pending.size() >= flush_pushes) return flush(A);
  return PSG_OK;
}

int psg_key_union(psg_ctx* c, int chl, const uint64_t* keys, size_t n) {
  if (!c || (n && !keys)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  if (n == 0) return PSG_OK;  // kv_vector.h:177: empty key list is ignored
  if (int rc = set_dev(c->device)) return rc;
  KeyRef k;
  if (int rc = c->new_keys(n, &k)) return rc;
  int rc = c->h2d(k->d, keys, 8 * n);
  if (rc == PSG_OK) rc = key_union_impl(c, chl, {k->d}, {(uint64_t)n});
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

int psg_key_union_batch(psg_ctx* c, int chl, const uint64_t* const* keys, const size_t* n,
                        int npush) {
  if (!c || npush < 0 || (npush && (!keys || !n))) return fail(PSG_ERR_ARG, "null argument");
  for (int p = 0; p < npush; ++p)
    if (n[p] && !keys[p]) return fail(PSG_ERR_ARG, "push %d: null keys", p);
  std::lock_guard<std::mutex> l(c->mu);
  if (int rc = set_dev(c->device)) return rc;
  std::vector<KeyRef> staged;
  std::vector<const uint64_t*> dp;
  std::vector<uint64_t> dn;
  int rc = PSG_OK;
  for (int p = 0; rc == PSG_OK && p < npush; ++p) {
    if (!n[p]) continue;
    KeyRef k;
    rc = c->new_keys(n[p], &k);
    if (rc == PSG_OK) rc = c->h2d(k->d, keys[p], 8 * n[p]);
    if (rc == PSG_OK) {
      staged.push_back(k);
      dp.push_back(k->d);
      dn.push_back(n[p]);
    }
  }
  if (rc == PSG_OK && !dp.empty()) rc = key_union_impl(c, chl, dp, dn);
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

int psg_key_size(psg_ctx* c, int chl, size_t* n) {
  if (!c || !n) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ch.find(chl);
  *n = it == c->ch.end() ? 0 : it->second.n;
  return PSG_OK;
}

int psg_key_copy(psg_ctx* c, int chl, size_t off, size_t n, uint64_t* out) {
  if (!c || (n && !out)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ch.find(chl);
  const size_t have = it == c->ch.end() ? 0 : it->second.n;
  if (off + n > have) return fail(PSG_ERR_ARG, "key copy out of range");
  if (n) memcpy(out, it->second.mirror() + off, 8 * n);
  return PSG_OK;
}

int psg_find_range(psg_ctx* c, int chl, uint64_t kb, uint64_t ke, size_t* lo,
                   size_t* hi) {
  if (!c || !lo || !hi) return fail(PSG_ERR_ARG, "null argument");
  if (ke < kb) return fail(PSG_ERR_ARG, "invalid key range");  // CHECK(bound.valid())
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ch.find(chl);
  if (it == c->ch.end() || it->second.n == 0) {
    *lo = *hi = 0;
    return PSG_OK;
  }
  const uint64_t* k = it->second.mirror();
  *lo = std::lower_bound(k, k + it->second.n, kb) - k;
  *hi = std::lower_bound(k, k + it->second.n, ke) - k;
  return PSG_OK;
}

int psg_value_assign(psg_ctx* c, int chl, const void* vals, size_t n) {
  if (!c || (n && !vals)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  if (int rc = set_dev(c->device)) return rc;
  Channel& C = c->ch[chl];
  const size_t sv = vsize(c->dtype);
  // the old array goes back to the pool (after any kernel reading it, a
  // device pull on a caller's stream included); the new one is written on
  // the copy stream once it is free
  if (int rc = c->chan_order(C, c->stream)) return rc;
  c->dev_put(C.d_vals, C.nvals * sv);
  C.d_vals = nullptr;
  C.nvals = 0;
  if (n) {
    if (int rc = c->dev_get(n * sv, &C.d_vals, c->copy)) return rc;
    C.nvals = n;
    if (int rc = c->h2d(C.d_vals, vals, n * sv)) return rc;
    // a device pull on another stream waits for the copy
    if (C.last)
      if (int rc = c->chan_mark(C, c->copy)) return rc;
  }
  return c->h2d_finish();
}

int psg_value_size(psg_ctx* c, int chl, size_t* n) {
  if (!c || !n) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ch.find(chl);
  *n = it == c->ch.end() ? 0 : it->second.nvals;
  return PSG_OK;
}

int psg_value_copy(psg_ctx* c, int chl, size_t off, size_t n, void* out) {
  if (!c || (n && !out)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ch.find(chl);
  const size_t have = it == c->ch.end() ? 0 : it->second.nvals;
  if (off + n > have) return fail(PSG_ERR_ARG, "value copy out of range");
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = c->join_copy()) return rc;
  if (int rc = c->chan_order(it->second, c->stream)) return rc;
  const size_t sv = vsize(c->dtype);
  if (n)
    HIP_TRY(hipMemcpyAsync(out, (char*)it->second.d_vals + off * sv, n * sv,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PSG_OK;
}

int psg_push(psg_ctx* c, int chl, int time, uint64_t kb, uint64_t ke,
             const uint64_t* keys, size_t n, int m, const void* const* vals) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  if (n == 0) return PSG_OK;  // kv_vector.h:90,177 -- empty push ignored
  if (!keys || !vals) return fail(PSG_ERR_ARG, "null keys/values");
  for (int i = 0; i < m && i < PSG_MAX_VALUE_ARRAYS; ++i)
    if (!vals[i]) return fail(PSG_ERR_ARG, "null value array %d", i);
  std::lock_guard<std::mutex> l(c->mu);
  if (int rc = set_dev(c->device)) return rc;
  size_t lo, hi;
  if (int rc = c->check_push(chl, time, kb, ke, n, m, &lo, &hi)) return rc;
  // Dense test ("back - front + 1 == n"): the push's first
  // key is server key a, its last is server key a + n - 1, and those n
  // server keys are n consecutive integers.  Then n strictly increasing
  // keys between them can only be exactly D[a, a + n): the merge reads no
  // keys (dense kernel, D's slice stands in for them) and the staged keys
  // are only checked strictly increasing, on the copy stream, into the
  // unmatched count psg_received reports -- the reference's
  // CHECK_EQ(matched, n) (kv_vector.h:192) in full.
  size_t a = 0;
  bool dense = false;
  if (n >= kDenseMinKeys) {
    const uint64_t* h = c->ch[chl].mirror();
    a = std::lower_bound(h + lo, h + hi, keys[0]) - h;
    dense = a + n <= hi && h[a] == keys[0] && h[a + n - 1] == keys[n - 1] &&
            h[a + n - 1] - h[a] == n - 1;
  }
  KeyRef k;
  int rc = PSG_OK;
  const void* kdev = nullptr;
  if (dense && c->zero_copy && host_pinned(keys, &kdev) && kdev && ((uintptr_t)kdev & 15u) == 0) {
    // pinned keys of a dense push: its order check reads them where they
    // are; nothing else needs them on the device (no HBM copy)
    k = std::make_shared<KeyBuf>();
    k->n = n;
    k->host = (const uint64_t*)kdev;
  } else {
    rc = c->new_keys(n, &k);
    // the keys and values of a pinned push in one zero-copy launch (a dense
    // push's keys are read by its check right away: not deferred)
    c->zc_group = !dense;
    if (rc == PSG_OK) rc = c->h2d(k->d, keys, 8 * n, !dense);
  }
  if (rc == PSG_OK) rc = c->push_values(chl, time, kb, ke, k, m, vals, nullptr, dense ? &a : nullptr);
  c->zc_group = false;
  if (!(c->flags & PSG_HOLD_BUFFERS)) {
    if (rc == PSG_OK) rc = c->zc_flush();
    else c->zc.n = 0;  // this push's queued copies only (its blocks went back)
  }
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

namespace {
int push_cached_impl(psg_ctx* c, int sender, int chl, int time, uint64_t kb, uint64_t ke,
                     unsigned kc, uint32_t sig, const uint64_t* keys, size_t nkeys, int m,
                     const void* const* vals, size_t nvals);
}

int psg_push_compressed(psg_ctx* c, int chl, int time, uint64_t kb, uint64_t ke,
                        const void* ckeys, size_t ckeys_bytes, int m, const void* const* cvals,
                        const size_t* cvals_bytes) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  if (m < 1 || m > PSG_MAX_VALUE_ARRAYS || !cvals || !cvals_bytes || (ckeys_bytes && !ckeys))
    return fail(PSG_ERR_ARG, "bad compressed push arguments");
  if (ckeys_bytes == 0) return PSG_OK;  // an empty key part: empty push, ignored
  // declared lengths (GetUncompressedLength); whole elements (:236)
  size_t klen = 0;
  if (int rc = psg_snappy_uncompressed_length(ckeys, ckeys_bytes, &klen)) return rc;
  if (klen % 8) return fail(PSG_ERR_SIZE, "key part of %zu bytes", klen);
  const size_t n = klen / 8;
  if (n == 0) return PSG_OK;
  const size_t sv = vsize(c->dtype);
  for (int i = 0; i < m; ++i) {
    size_t vl = 0;
    if (!cvals[i] || !cvals_bytes[i]) return fail(PSG_ERR_SIZE, "empty value part %d", i);
    if (int rc = psg_snappy_uncompressed_length(cvals[i], cvals_bytes[i], &vl)) return rc;
    if (vl != n * sv)  // CHECK_EQ(recv_data.size(), recv_key.size()) kv_vector.h:187
      return fail(PSG_ERR_SIZE, "value part %d: %zu bytes for %zu keys", i, vl, n);
  }
  std::lock_guard<std::mutex> l(c->mu);
  if (int rc = set_dev(c->device)) return rc;
  size_t lo, hi;
  if (int rc = c->check_push(chl, time, kb, ke, n, m, &lo, &hi)) return rc;
  // staging block: the m + 1 compressed parts back to back; they are
  // decoded right before the merge that needs them (psg_ctx::flush), with
  // every other compressed push pending then, in one launch
  const int np = m + 1;
  // part i at soff[i], 16-B aligned (the zero-copy read needs both ends
  // aligned), plen[i] bytes
  std::vector<uint64_t> soff(np + 1, 0), plen(np, 0);
  plen[0] = ckeys_bytes;
  for (int i = 0; i < m; ++i) plen[i + 1] = cvals_bytes[i];
  for (int i = 0; i < np; ++i) soff[i + 1] = align_up(soff[i] + plen[i], 16);
  const size_t tb = align_up(soff[np], 256);
  void* blk = nullptr;
  if (int rc = c->dev_get(tb, &blk, c->copy)) return rc;
  KeyRef k;
  void* vblock = nullptr;
  const size_t vb = align_up(sv * n, 256);
  int rc = c->new_keys(n, &k);
  if (rc == PSG_OK) rc = c->dev_get(m * vb, &vblock, c->copy);
  char* b = (char*)blk;
  // the parts in one zero-copy launch when the caller's buffers are pinned
  c->zc_group = true;
  if (rc == PSG_OK) rc = c->h2d(b, ckeys, ckeys_bytes, true);
  for (int i = 0; rc == PSG_OK && i < m; ++i) rc = c->h2d(b + soff[i + 1], cvals[i], cvals_bytes[i], true);
  c->zc_group = false;
  if (rc == PSG_OK && !(c->flags & PSG_HOLD_BUFFERS)) rc = c->zc_flush();
  // the caller's buffers are free once their copies land (unless held)
  if (rc == PSG_OK) rc = c->h2d_finish();
  if (rc != PSG_OK) {
    if (!(c->flags & PSG_HOLD_BUFFERS)) c->zc.n = 0;  // this push's queued copies only
    (void)hipStreamSynchronize(c->copy);
    c->dev_put(blk, tb);
    c->dev_put(vblock, m * vb);
    return rc;
  }
  PendingPush cp;
  cp.cparts = np;
  for (int i = 0; i < np; ++i) {
    cp.cbeg[i] = (uint64_t)(b + soff[i]);
    cp.cend[i] = (uint64_t)(b + soff[i] + plen[i]);
    cp.cdst[i] = i == 0 ? (uint64_t)k->d : (uint64_t)((char*)vblock + (i - 1) * vb);
    cp.ccap[i] = i == 0 ? (uint64_t)klen : (uint64_t)(n * sv);
  }
  return c->push_values(chl, time, kb, ke, k, m, nullptr, vblock, nullptr, blk, tb, &cp);
}

int psg_push_cached(psg_ctx* c, int sender, int chl, int time, uint64_t kb, uint64_t ke,
                    unsigned kc, uint32_t sig, const uint64_t* keys, size_t nkeys, int m,
                    const void* const* vals, size_t nvals) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  const int rc = push_cached_impl(c, sender, chl, time, kb, ke, kc, sig, keys, nkeys, m, vals,
                                  nvals);
  const int rf = c->h2d_finish();
  return rc ? rc : rf;
}

namespace {
int push_cached_impl(psg_ctx* c, int sender, int chl, int time, uint64_t kb, uint64_t ke,
                     unsigned kc, uint32_t sig, const uint64_t* keys, size_t nkeys, int m,
                     const void* const* vals, size_t nvals) {
  if ((kc & PSG_KC_KEYS) && nkeys && !keys) return fail(PSG_ERR_ARG, "null keys");
  if (m < 0 || m > PSG_MAX_VALUE_ARRAYS || (m > 0 && !vals)) return fail(PSG_ERR_ARG, "m=%d", m);
  for (int i = 0; i < m; ++i)
    if (nvals && !vals[i]) return fail(PSG_ERR_ARG, "null value array %d", i);
  if (int rc = set_dev(c->device)) return rc;
  const CacheKey ck{sender, chl, kb, ke};
  KeyRef k;  // the message's keys, resident
  bool sigcheck = false;  // the carried signature checked on the device
  if (!(kc & PSG_KC_SIG)) {
    // no signature: the cache entry of (channel, range) is dropped
    // (remote_node.cc:143-156) and the message's own keys are used
    c->kcache.erase(ck);
    if ((kc & PSG_KC_KEYS) && nkeys) {
      if (int rc = c->new_keys(nkeys, &k)) return rc;
      if (int rc = c->h2d(k->d, keys, 8 * nkeys)) return rc;
    }
  } else if (kc & PSG_KC_KEYS) {
    // keys carried: check the signature, store them (remote_node.cc:161-171)
    if (nkeys) {
      if (int rc = c->new_keys(nkeys, &k)) return rc;
      if (int rc = c->h2d(k->d, keys, 8 * nkeys)) return rc;
    }
    uint32_t got = 0;  // crc32c::Value of no bytes
    // with values (m > 0) the check runs on the device and a mismatch is
    // reported by psg_received (no host wait); the entry stores the keys as
    // pending on that check: a restore waits for its result and fails (and
    // drops the entry) if it failed.  A key-only message merges into the
    // channel's keys at once, so it is checked before that
    if (nkeys && m > 0) {
      sigcheck = true;  // launched below, into the entry's and the aggregate's counters
      got = sig;
    } else if (nkeys) {
      c->h_small[8] = 0;
      c->h_small[9] = 8 * nkeys;
      HIP_TRY(hipMemcpyAsync(c->d_small + 8, c->h_small + 8, 16, hipMemcpyHostToDevice, c->copy));
      HIP_TRY(psg::launch_crc32c((const uint8_t*)k->d, (const uint64_t*)(c->d_small + 8), 1,
                                 PSG_MAX_SIG_LEN, nullptr, (uint32_t*)(c->d_small + 10), c->copy));
      HIP_TRY(hipMemcpyAsync(c->h_small + 10, c->d_small + 10, 8, hipMemcpyDeviceToHost, c->copy));
      HIP_TRY(hipStreamSynchronize(c->copy));
      got = (uint32_t)c->h_small[10];
    }
    if (got != sig)  // CHECK_EQ(crc32c(key), sig) remote_node.cc:163
      return fail(PSG_ERR_SIGNATURE, "key signature %08x != carried %08x", got, sig);
    CacheEntry& e = c->kcache[ck];
    e.sig = sig;
    e.keys = k;
    e.chk.reset();
  } else {
    // keys restored from the cache (remote_node.cc:172-176)
    auto it = c->kcache.find(ck);
    if (it != c->kcache.end() && it->second.chk) {
      // stored by a keyed message whose device check has not been read yet
      bool ok = false;
      if (int rc = c->sig_check_result(it->second.chk, &ok)) return rc;
      if (!ok) {
        const uint32_t bad = it->second.sig;
        c->kcache.erase(it);
        return fail(PSG_ERR_SIGNATURE,
                    "key cache of channel %d [%llu,%llu): the stored keys did not match their "
                    "signature %08x",
                    chl, (unsigned long long)kb, (unsigned long long)ke, bad);
      }
      it->second.chk.reset();
    }
    const uint32_t have = it == c->kcache.end() ? 0u : it->second.sig;
    if (sig != have)  // CHECK_EQ(sig, cache.first)
      return fail(PSG_ERR_SIGNATURE, "key cache of channel %d [%llu,%llu): signature %08x != %08x",
                  chl, (unsigned long long)kb, (unsigned long long)ke, sig, have);
    if (it != c->kcache.end()) k = it->second.keys;
  }
  // the stored entry's pending check (keys carried with values): ONE device
  // CRC of the keys, counted into the entry's counter (a later restore waits
  // for it) and into the aggregate's (psg_received reports a mismatch).  If
  // the message is refused before its aggregate exists, the check still
  // runs, into the entry's counter alone: the entry is never restorable
  // unchecked
  auto store_check = [&](unsigned long long* agg) -> int {
    auto it = c->kcache.find(ck);
    if (it == c->kcache.end() || it->second.keys != k) return PSG_OK;  // erased meanwhile
    SigCheckRef pend;
    if (int rc = c->sig_check_pending(k, sig, &pend, agg)) return rc;
    it->second.chk = pend;
    return PSG_OK;
  };
  if (kc & PSG_KC_ERASE) c->kcache.erase(ck);  // remote_node.cc:183
  const size_t n = k ? k->n : 0;
  if (n == 0) return PSG_OK;  // kv_vector.h:90,177: no keys, message ignored
  if (m == 0) {
    // key-only message: setUnion with the (possibly restored) keys, on the device
    return key_union_impl(c, chl, {k->d}, {(uint64_t)n});
  }
  if (nvals != n) {  // CHECK_EQ(recv_data.size(), recv_key.size()) kv_vector.h:108,187
    if (sigcheck) (void)store_check(nullptr);
    return fail(PSG_ERR_SIZE, "%zu values for %zu keys", nvals, n);
  }
  size_t lo, hi;
  if (int rc = c->check_push(chl, time, kb, ke, n, m, &lo, &hi)) {
    if (sigcheck) (void)store_check(nullptr);
    return rc;
  }
  if (sigcheck) {  // on `copy` after the key copy
    Aggregate* A = nullptr;
    if (int rc = c->aggregate_for(chl, time, kb, ke, m, &A)) {
      (void)store_check(nullptr);
      return rc;
    }
    if (int rc = store_check(A->d_bad + 2)) return rc;
    if (!c->kcache.count(ck))  // the entry was erased (PSG_KC_ERASE): the aggregate's check alone
      HIP_TRY(psg::launch_sig_check((const uint8_t*)k->d, 8 * n, PSG_MAX_SIG_LEN, sig,
                                    A->d_bad + 2, c->copy));
  }
  return c->push_values(chl, time, kb, ke, k, m, vals);
}

}  // namespace

int psg_key_cache_clear(psg_ctx* c, int sender) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  for (auto it = c->kcache.begin(); it != c->kcache.end();)
    it = (sender < 0 || it->first.sender == sender) ? c->kcache.erase(it) : std::next(it);
  return PSG_OK;
}

int psg_key_cache_bytes(psg_ctx* c, int sender, size_t* bytes) {
  if (!c || !bytes) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  size_t b = 0;
  for (const auto& kv : c->kcache)
    if ((sender < 0 || kv.first.sender == sender) && kv.second.keys) b += kv.second.keys->bytes;
  *bytes = b;
  return PSG_OK;
}

int psg_received_shape(psg_ctx* c, int time, int* m, size_t* lo, size_t* hi) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->agg.find(time);
  if (it == c->agg.end()) return fail(PSG_ERR_NO_TIME, "no data received at time %d", time);
  if (m) *m = it->second.m;
  if (lo) *lo = it->second.lo;
  if (hi) *hi = it->second.hi;
  return PSG_OK;
}

int psg_received(psg_ctx* c, int time, int m, void* const* out) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->agg.find(time);
  if (it == c->agg.end()) return fail(PSG_ERR_NO_TIME, "no data received at time %d", time);
  if (int rc = set_dev(c->device)) return rc;
  Aggregate& A = it->second;
  if (m != A.m || !out) return fail(PSG_ERR_ARG, "expected %d output arrays", A.m);
  const size_t len = A.hi - A.lo, sv = vsize(c->dtype);
  // the whole aggregate in one launch into pinned caller arrays: the merge
  // kernel writes the sums there itself (no separate readback)
  bool direct = c->zero_copy && A.folded == 0 && !A.pending.empty() &&
                A.pending.size() <= c->flush_pushes && len > 0;
  void* dev_out[psg::kMaxM] = {};
  for (int i = 0; direct && i < A.m; ++i) {
    const void* d = nullptr;
    direct = host_pinned(out[i], &d) && d && ((uintptr_t)d & 15u) == 0;
    dev_out[i] = (void*)d;
  }
  const bool pend = !A.pending.empty();
  int rc = c->flush(A, direct ? dev_out : nullptr, direct ? c->h_small : nullptr);
  for (int i = 0; !direct && rc == PSG_OK && i < A.m && len; ++i)
    rc = c->d2h(out[i], A.d_out[i], len * sv);
  unsigned long long bad = 0;
  unsigned long long corrupt = 0, badsig = 0;
  if (rc == PSG_OK && !(direct && pend)) rc = c->d2h(c->h_small, A.d_bad, kBadBytes);
  if (rc == PSG_OK) {
    hipError_t e = hipEventRecord(c->done_ev, c->stream);
    if (e == hipSuccess) e = spin_wait(c->done_ev);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "received: %s", hipGetErrorString(e));
    bad = c->h_small[0];
    corrupt = c->h_small[1];
    badsig = c->h_small[2];
  }
  const unsigned long long want = A.expected_total;
  c->drop(A);
  c->agg.erase(it);
  if (rc) return rc;
  if (corrupt)  // Van::recv's CHECK on uncompressFrom (shared_array_inl.h:236)
    return fail(PSG_ERR_ARG, "time %d: %llu compressed parts failed to decode", time, corrupt);
  if (badsig)  // cacheKeyRecver's CHECK_EQ(crc32c(key), sig) (remote_node.cc:163)
    return fail(PSG_ERR_SIGNATURE, "time %d: %llu pushes' keys do not match their signature",
                time, badsig);
  if (bad)
    return fail(PSG_ERR_UNMATCHED, "time %d: matched %llu of %llu pushed keys", time,
                want - bad, want);
  return PSG_OK;
}

int psg_darling_init(psg_ctx* c, int chl, double delta_init) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  if (c->dtype != PSG_F64) return fail(PSG_ERR_ARG, "Darling needs a PSG_F64 context");
  if (int rc = set_dev(c->device)) return rc;
  Channel& C = c->ch[chl];
  if (C.dn != C.n) {
    c->dev_put(C.d_delta, 8 * C.dn);
    c->dev_put(C.d_active, 4 * ((C.dn + 31) / 32));
    C.d_delta = nullptr;
    C.d_active = nullptr;
    C.dn = 0;
    if (C.n) {
      if (int rc = c->dev_get(8 * C.n, (void**)&C.d_delta, c->stream)) return rc;
      if (int rc = c->dev_get(4 * ((C.n + 31) / 32), (void**)&C.d_active, c->stream)) return rc;
    }
    C.dn = C.n;
  }
  HIP_TRY(psg::launch_darling_init(C.d_delta, C.d_active, C.dn, delta_init, c->stream));
  return PSG_OK;
}

int psg_darling_reset_active(psg_ctx* c, int chl) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ch.find(chl);
  if (it == c->ch.end() || !it->second.d_active)
    return fail(PSG_ERR_ARG, "channel %d: no Darling state (psg_darling_init)", chl);
  if (int rc = set_dev(c->device)) return rc;
  HIP_TRY(psg::launch_bitmap_fill(it->second.d_active, it->second.dn, c->stream));
  return PSG_OK;
}

int psg_darling_update(psg_ctx* c, int chl, int time, const psg_darling_param* p,
                       double* violation) {
  if (!c || !p) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->agg.find(time);
  if (it == c->agg.end()) return fail(PSG_ERR_NO_TIME, "no data received at time %d", time);
  if (int rc = set_dev(c->device)) return rc;
  Aggregate& A = it->second;
  if (A.chl != chl) return fail(PSG_ERR_CHANNEL, "time %d: channel %d != %d", time, A.chl, chl);
  if (A.m != 2) return fail(PSG_ERR_ARG, "Darling needs 2 aggregates (G, U), time %d has %d",
                            time, A.m);  // CHECK_EQ(data.size(), 2) darling.cc:253
  Channel& C = c->ch[chl];
  if (C.nvals != C.n || C.dn != C.n)
    return fail(PSG_ERR_SIZE, "channel %d: %zu keys, %zu values, Darling state of %zu", chl,
                C.n, C.nvals, C.dn);
  int rc = c->flush(A);
  if (rc == PSG_OK) rc = c->chan_order(C, c->stream);
  if (rc == PSG_OK) {
    const psg::DarlingParam P{p->eta, p->lambda, p->kkt_filter_threshold, p->delta_max};
    unsigned long long* dv = c->d_small + 4;
    hipError_t e = psg::launch_darling((const double*)A.d_out[0], (const double*)A.d_out[1],
                                       (double*)C.d_vals, C.d_delta, C.d_active, A.lo,
                                       A.hi - A.lo, P, A.d_bad, c->d_vio_slots, dv, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(c->h_small + 4, dv, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(c->h_small + 5, A.d_bad, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "darling update: %s", hipGetErrorString(e));
  }
  const unsigned long long bad = rc == PSG_OK ? c->h_small[5] : 0, want = A.expected_total;
  if (rc == PSG_OK && violation) memcpy(violation, c->h_small + 4, 8);
  c->drop(A);
  c->agg.erase(it);
  if (rc) return rc;
  if (bad)
    return fail(PSG_ERR_UNMATCHED, "time %d: matched %llu of %llu pushed keys", time,
                want - bad, want);
  return PSG_OK;
}

int psg_darling_state(psg_ctx* c, int chl, size_t off, size_t n, double* delta, uint8_t* active,
                      size_t* nnz_active) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ch.find(chl);
  if (it == c->ch.end() || !it->second.d_active)
    return fail(PSG_ERR_ARG, "channel %d: no Darling state (psg_darling_init)", chl);
  const Channel& C = it->second;
  if (off + n > C.dn) return fail(PSG_ERR_ARG, "Darling state copy out of range");
  if (int rc = set_dev(c->device)) return rc;
  std::vector<uint32_t> bits;
  if (active && n) bits.resize((off + n + 31) / 32 - off / 32);
  if (delta && n)
    HIP_TRY(hipMemcpyAsync(delta, C.d_delta + off, 8 * n, hipMemcpyDeviceToHost, c->stream));
  if (!bits.empty())
    HIP_TRY(hipMemcpyAsync(bits.data(), C.d_active + off / 32, 4 * bits.size(),
                           hipMemcpyDeviceToHost, c->stream));
  if (nnz_active) {
    HIP_TRY(hipMemsetAsync(c->d_small + 6, 0, 8, c->stream));
    HIP_TRY(psg::launch_popcount(C.d_active, (C.dn + 31) / 32, c->d_small + 6, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_small + 6, c->d_small + 6, 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; active && i < n; ++i) {
    const size_t k = off + i;
    active[i] = (uint8_t)((bits[k / 32 - off / 32] >> (k % 32)) & 1u);
  }
  if (nnz_active) *nnz_active = (size_t)c->h_small[6];
  return PSG_OK;
}

int psg_gather(psg_ctx* c, int chl, const uint64_t* keys, size_t n, void* out,
               size_t* matched) {
  if (!c || (n && (!keys || !out))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  if (matched) *matched = 0;
  if (n == 0) return PSG_OK;  // kv_vector.h:218
  if (int rc = set_dev(c->device)) return rc;
  Channel& C = c->ch[chl];
  if (C.n != C.nvals)  // CHECK_EQ(key_[ch].size(), val_[ch].size()) kv_vector.h:220
    return fail(PSG_ERR_SIZE, "channel %d: %zu keys but %zu values", chl, C.n, C.nvals);
  const size_t sv = vsize(c->dtype);
  if (int rc = c->ensure_scratch(align_up(8 * n, 256) + n * sv)) return rc;
  uint64_t* d_req = (uint64_t*)c->scratch;
  void* d_out = (char*)c->scratch + align_up(8 * n, 256);
  if (int rc = c->h2d(d_req, keys, 8 * n)) return rc;
  if (int rc = c->join_copy()) return rc;
  if (int rc = c->chan_order(C, c->stream)) return rc;
  HIP_TRY(hipMemsetAsync(c->d_small, 0, 16, c->stream));
  HIP_TRY(psg::launch_check_sorted(d_req, n, c->d_small + 1, c->stream, false));
  HIP_TRY(psg::launch_gather(c->dtype, C.d_keys, C.n, C.d_vals, d_req, n, d_out,
                             c->d_small, c->stream));
  HIP_TRY(hipMemcpyAsync(out, d_out, n * sv, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small, c->d_small, 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // getValue walks the request with the merge of oldMatch (kv_vector.h:
  // 222-224), whose contract is a sorted request (message.h:248-264)
  if (int rc = c->h2d_finish()) return rc;
  if (c->h_small[1]) return fail(PSG_ERR_UNSORTED, "gather: request keys not sorted");
  if (matched) *matched = (size_t)c->h_small[0];
  return PSG_OK;
}

int psg_gather_compressed(psg_ctx* c, int chl, const uint64_t* keys, size_t n, void* out,
                          size_t cap, size_t* out_bytes, size_t* matched) {
  if (!c || !out || !out_bytes || (n && !keys)) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  const size_t sv = vsize(c->dtype), raw = n * sv;
  const size_t room = psg_snappy_max_compressed_length(raw);
  if (raw > 0xffffffffull) return fail(PSG_ERR_SIZE, "gather: a value part of %zu bytes", raw);
  if (cap < room)
    return fail(PSG_ERR_SIZE, "gather: room for %zu bytes, %zu values may need %zu", cap, n, room);
  if (matched) *matched = 0;
  *out_bytes = 0;
  if (n == 0) {  // the stream of an empty part: its preamble
    *(uint8_t*)out = 0;
    *out_bytes = 1;
    return PSG_OK;
  }
  if (int rc = set_dev(c->device)) return rc;
  Channel& C = c->ch[chl];
  if (C.n != C.nvals)  // CHECK_EQ(key_[ch].size(), val_[ch].size()) kv_vector.h:220
    return fail(PSG_ERR_SIZE, "channel %d: %zu keys but %zu values", chl, C.n, C.nvals);
  // one pooled block: request keys | offsets and clen | values | stream | scratch
  const size_t o_off = align_up(8 * n, 256), o_val = o_off + 256;
  const size_t o_dst = o_val + align_up(raw, 256), o_scr = o_dst + align_up(room, 256);
  const size_t bytes = o_scr + psg::snappy_compress_scratch_bytes(raw, 1);
  void* blk = nullptr;
  if (int rc = c->dev_get(bytes, &blk, c->copy)) return rc;
  char* b = (char*)blk;
  uint64_t* d_req = (uint64_t*)b;
  uint64_t* d_off = (uint64_t*)(b + o_off);  // soff[2], doff[1], clen[1]
  const uint64_t h_off[3] = {0, (uint64_t)raw, 0};
  int rc = c->h2d(d_req, keys, 8 * n);
  if (rc == PSG_OK) rc = c->h2d(d_off, h_off, sizeof h_off);
  if (rc == PSG_OK) rc = c->join_copy();
  if (rc == PSG_OK) rc = c->chan_order(C, c->stream);
  hipError_t e = hipSuccess;
  if (rc == PSG_OK) {
    e = hipMemsetAsync(c->d_small, 0, 16, c->stream);
    if (e == hipSuccess) e = psg::launch_check_sorted(d_req, n, c->d_small + 1, c->stream, false);
    if (e == hipSuccess)
      e = psg::launch_gather(c->dtype, C.d_keys, C.n, C.d_vals, d_req, n, b + o_val, c->d_small,
                             c->stream);
    if (e == hipSuccess)
      e = psg::launch_snappy_compress((const uint8_t*)b + o_val, d_off, 1, (uint8_t*)b + o_dst,
                                      d_off + 2, d_off + 3, b + o_scr, c->stream);
    // the stream's length first, then that many bytes
    if (e == hipSuccess)
      e = hipMemcpyAsync(c->h_small, c->d_small, 16, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(c->h_small + 12, d_off + 3, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "gather: %s", hipGetErrorString(e));
  }
  const int rf = c->h2d_finish();
  if (rc == PSG_OK) rc = rf;
  if (rc == PSG_OK && c->h_small[1]) rc = fail(PSG_ERR_UNSORTED, "gather: request keys not sorted");
  const size_t len = (size_t)c->h_small[12];
  if (rc == PSG_OK && (len == 0 || len > room))
    rc = fail(PSG_ERR_DEVICE, "gather: a stream of %zu bytes for %zu values", len, n);
  if (rc == PSG_OK) rc = c->d2h(out, b + o_dst, len);
  if (rc == PSG_OK && (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    rc = fail(PSG_ERR_DEVICE, "gather: %s", hipGetErrorString(e));
  c->dev_put(blk, bytes);
  if (rc) return rc;
  *out_bytes = len;
  if (matched) *matched = (size_t)c->h_small[0];
  return PSG_OK;
}

}  // extern "C"
