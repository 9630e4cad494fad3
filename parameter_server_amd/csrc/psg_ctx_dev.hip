// psg_ctx_dev.hip -- the device-array forms of the server context
// (psg_push_dev, psg_pull_dev, psg_darling_update_dev, psg_darling_progress,
// psg_dev_status; include/psg.h) and their kernels: the intake of a device
// message and the server sums of Darling::evaluateProgress.  The pull kernel
// sits beside the gather it shares its code with (psg_kernels.hip), the
// update's violation fold beside darling_kernel (psg_darling.hip).
//
// Ordering (include/psg.h, "Ordering rule").  A device push is copied into the
// context's pool blocks by one launch on the CALLER's stream; `copy` then
// waits for an event recorded behind that launch, and every fold joins `copy`
// (psg_ctx::join_copy) -- so the fold runs after the intake, and whatever the
// caller enqueues on its stream afterwards runs after it too.  A channel's
// values carry an event chain (Channel::last / last_s, as Filter's and
// Ftrl's): each pull and update waits for the event of the operation called
// before it when their streams differ.  No call here waits on the host except
// the two that say so (psg_darling_progress, psg_dev_status).
#include "psg_ctx.h"
#include "psg_device.h"

namespace psg {
namespace {

using dev::u32x4;

template <typename T>
__device__ __forceinline__ void copy_elems(const char* __restrict__ s, char* __restrict__ d,
                                           uint64_t n, uint64_t tid, uint64_t stride) {
  for (uint64_t u = tid; u < n; u += stride) ((T*)d)[u] = ((const T*)s)[u];
}

// Every workgroup walks each array of the message in turn.  The pool's blocks
// start on a 16-byte bound; a caller's array need not (U sits 8 bytes off one
// whenever the block has an odd number of columns).  Both ends on a bound:
// 16-B loads and stores, 4 in flight per thread, and the elements after the
// last whole 16 bytes one by one.  Otherwise element loads and stores
// throughout.
__global__ __launch_bounds__(256) void intake_kernel(IntakeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  const uint64_t tid = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  for (uint32_t c = 0; c < a.n; ++c) {
    const char* __restrict__ s = (const char*)a.src[c];
    char* __restrict__ d = (char*)a.dst[c];
    const uint64_t len = a.len[c];
    const bool vec = (((uintptr_t)s | (uintptr_t)d) & 15u) == 0;
    const uint64_t n16 = vec ? len / 16 : 0, done = 16 * n16;
    if (a.esz[c] == 8) copy_elems<uint64_t>(s + done, d + done, (len - done) / 8, tid, stride);
    else copy_elems<uint32_t>(s + done, d + done, (len - done) / 4, tid, stride);
    const u32x4* __restrict__ sv = (const u32x4*)s;
    u32x4* __restrict__ dv = (u32x4*)d;
    for (uint64_t u = tid; u < n16; u += 4 * stride) {
      u32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (u + j * stride < n16) v[j] = __builtin_nontemporal_load(sv + u + j * stride);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (u + j * stride < n16) dv[u + j * stride] = v[j];
    }
  }
  // a slice claim: the keys are not copied but compared with the server keys
  // they claim to be; one atomic per wave that saw a difference
  if (a.nclaim) {
    uint32_t cnt = 0;
    for (uint64_t i = tid; i < a.nclaim; i += stride) cnt += a.claim_keys[i] != a.D[i] ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt)
      __hip_atomic_fetch_add(a.bad, (unsigned long long)cnt, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

// evaluateProgress (darling.cc:538-555): a weight counts unless it is
// inactive(w), which is w != w -- any NaN, not only kInactiveValue_'s bits --
// or zero (-0.0 == 0).  psum[workgroup] = the tree sum of its 256 |w|,
// pcnt[workgroup] = its count.
__global__ __launch_bounds__(256) void progress_kernel(const double* __restrict__ w, uint64_t n,
                                                       double* __restrict__ psum,
                                                       unsigned long long* __restrict__ pcnt) {
  __shared__ double s[256];
  __shared__ uint32_t wc[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  bool live = false;
  double a = 0.0;
  if (i < n) {
    const double x = w[i];
    live = x == x && x != 0;
    a = live ? fabs(x) : 0.0;
  }
  const unsigned long long m = __ballot(live);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  dev::block_tree_sum(a, s);
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = s[0];
    pcnt[blockIdx.x] = (unsigned long long)wc[0] + wc[1] + wc[2] + wc[3];
  }
}

// thread t adds partials t, t + 256, ... one after the other; then the tree
// (objv_kernel's order: it depends on n alone)
__global__ __launch_bounds__(256) void progress_final_kernel(
    const double* __restrict__ psum, const unsigned long long* __restrict__ pcnt, uint64_t nparts,
    unsigned long long* __restrict__ res) {
  __shared__ double s[256];
  __shared__ unsigned long long wc[4];
  double a = 0.0;
  unsigned long long c = 0;
  for (uint64_t p = threadIdx.x; p < nparts; p += 256) {
    a += psum[p];
    c += pcnt[p];
  }
  for (int o = 32; o > 0; o >>= 1) c += (unsigned long long)__shfl_xor((long long)c, o, 64);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
  dev::block_tree_sum(a, s);
  if (threadIdx.x == 0) {
    res[0] = wc[0] + wc[1] + wc[2] + wc[3];
    res[1] = (unsigned long long)__double_as_longlong(s[0]);
  }
}

}  // namespace

hipError_t launch_intake(const IntakeArgs& a, hipStream_t stream) {
  uint64_t bytes = 8 * a.nclaim;
  for (uint32_t c = 0; c < a.n; ++c) bytes += a.len[c];
  if (bytes == 0) return hipSuccess;
  // by bytes: 16 KB per workgroup (256 threads x 4 x 16 B); a block-sized
  // message is one workgroup
  uint64_t blocks = (bytes + 16383) / 16384;
  blocks = blocks > 256 ? 256 : blocks;
  hipLaunchKernelGGL(intake_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_progress(const double* w, uint64_t n, unsigned long long* partial,
                           unsigned long long* res, hipStream_t stream) {
  const uint64_t parts = progress_parts(n);
  double* psum = (double*)partial;
  unsigned long long* pcnt = partial + parts;
  if (parts)
    hipLaunchKernelGGL(progress_kernel, dim3((uint32_t)parts), dim3(256), 0, stream, w, n, psum,
                       pcnt);
  hipLaunchKernelGGL(progress_final_kernel, dim3(1), dim3(256), 0, stream, psum, pcnt, parts, res);
  return hipGetLastError();
}

}  // namespace psg

namespace {

// d_small / h_small words of the device forms
constexpr int kErrSkipped = 16;  // updates skipped: a push of their block did not match
constexpr int kErrUnsorted = 17; // order violations of pull requests
constexpr int kProgVio = 19;     // host side only: the channel's violation word
constexpr int kProgRes = 20;     // count, sum bits
constexpr int kProgActive = 22;  // popcount of the active set

// the channel's device words ([0] accumulated violation, [1..2] the pull
// kernel's count and ticket), zeroed on the context's stream when first needed
int chan_words(psg_ctx* c, Channel& C) {
  if (C.d_dev) return PSG_OK;
  if (int rc = c->dev_get(kChanWordBytes, (void**)&C.d_dev, c->stream)) return rc;
  HIP_TRY(hipMemsetAsync(C.d_dev, 0, kChanWordBytes, c->stream));
  // the channel's first event also stands for the values assigned so far,
  // whose copy may still run on `copy` (psg_value_assign marks later ones)
  if (int rc = c->join_copy()) return rc;
  if (int rc = c->chan_order(C, c->stream)) return rc;
  return c->chan_mark(C, c->stream);
}

// the context's stream behind every channel's last operation: what a reader
// of the deferred-error words waits for
int order_all(psg_ctx* c) {
  for (auto& kv : c->ch)
    if (int rc = c->chan_order(kv.second, c->stream)) return rc;
  return PSG_OK;
}

// The deferred error of the device forms as just read into h_small: reported
// once by the synchronising call that read it, then cleared.
int report_deferred(psg_ctx* c) {
  const unsigned long long skipped = c->h_small[kErrSkipped], unsorted = c->h_small[kErrUnsorted];
  if (!skipped && !unsorted) return PSG_OK;
  HIP_TRY(hipMemsetAsync(c->d_small + kErrSkipped, 0, 16, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (skipped)
    return fail(PSG_ERR_UNMATCHED, "%llu Darling updates were skipped: a push of their block "
                "had keys that are not server keys of its range", skipped);
  return fail(PSG_ERR_UNSORTED, "%llu key pairs of device pull requests not sorted", unsorted);
}

}  // namespace

extern "C" {

int psg_push_dev(psg_ctx* c, int chl, int time, uint64_t kb, uint64_t ke,
                 const uint64_t* keys_dev, size_t n, int m, const void* const* vals_dev,
                 size_t slice, void* stream) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  if (n == 0) return PSG_OK;  // kv_vector.h:90,177 -- empty push ignored
  if (!keys_dev || !vals_dev) return fail(PSG_ERR_ARG, "null keys/values");
  for (int i = 0; i < m && i < PSG_MAX_VALUE_ARRAYS; ++i)
    if (!vals_dev[i]) return fail(PSG_ERR_ARG, "null value array %d", i);
  std::lock_guard<std::mutex> l(c->mu);
  if (int rc = set_dev(c->device)) return rc;
  size_t lo, hi;
  if (int rc = c->check_push(chl, time, kb, ke, n, m, &lo, &hi)) return rc;
  const bool claim = slice != PSG_NO_SLICE;
  if (claim && (slice < lo || slice > hi || n > hi - slice))
    return fail(PSG_ERR_ARG, "slice claim [%zu, %zu + %zu) outside the range [%zu, %zu)", slice,
                slice, n, lo, hi);
  hipStream_t s = (hipStream_t)stream;
  const size_t sv = vsize(c->dtype), vb = align_up(sv * n, 256);
  KeyRef k;
  if (claim) {
    // D's slice stands in for the keys (push_values' slice path): no copy
    k = std::make_shared<KeyBuf>();
    k->n = n;
  } else if (int rc = c->new_keys(n, &k, s)) {
    return rc;
  }
  void* vblock = nullptr;
  if (int rc = c->dev_get(m * vb, &vblock, s)) return rc;
  // the aggregate first: a claim's differences are added to its counter
  Aggregate* A = nullptr;
  int rc = c->aggregate_for(chl, time, kb, ke, m, &A);
  psg::IntakeArgs a;
  if (rc == PSG_OK) {
    if (claim) {
      a.claim_keys = keys_dev;
      a.D = c->ch[chl].d_keys + slice;
      a.nclaim = n;
      a.bad = A->d_bad;
      // the counter was zeroed on `copy` when the aggregate was made: the
      // caller's stream waits for that on the device
      if (hipEventRecord(c->copy_ev, c->copy) != hipSuccess ||
          hipStreamWaitEvent(s, c->copy_ev, 0) != hipSuccess)
        rc = fail(PSG_ERR_DEVICE, "push_dev: ordering the claim check");
    } else {
      a.src[a.n] = keys_dev;
      a.dst[a.n] = k->d;
      a.len[a.n] = 8 * n;
      a.esz[a.n++] = 8;
    }
    for (int i = 0; i < m; ++i) {
      a.src[a.n] = vals_dev[i];
      a.dst[a.n] = (char*)vblock + i * vb;
      a.len[a.n] = sv * n;
      a.esz[a.n++] = (uint32_t)sv;
    }
  }
  // the intake on the caller's stream; `copy`, which every fold joins, waits
  // for it
  hipEvent_t e = nullptr;
  if (rc == PSG_OK) rc = c->event(&e);
  if (rc == PSG_OK) {
    hipError_t he = psg::launch_intake(a, s);
    if (he == hipSuccess) he = hipEventRecord(e, s);
    if (he == hipSuccess) he = hipStreamWaitEvent(c->copy, e, 0);
    if (he != hipSuccess) rc = fail(PSG_ERR_DEVICE, "push_dev: %s", hipGetErrorString(he));
  }
  if (e) c->free_ev.push_back(e);
  if (rc != PSG_OK) {
    (void)hipStreamSynchronize(s);  // the blocks go back behind whatever was enqueued
    c->dev_put(vblock, m * vb);
    return rc;
  }
  return c->push_values(chl, time, kb, ke, k, m, nullptr, vblock, claim ? &slice : nullptr);
}

int psg_pull_dev(psg_ctx* c, int chl, const uint64_t* keys_dev, size_t n, void* out_dev,
                 unsigned long long* matched_dev, void* stream) {
  if (!c || (n && (!keys_dev || !out_dev))) return fail(PSG_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> l(c->mu);
  if (n == 0) return PSG_OK;  // kv_vector.h:218
  if (int rc = set_dev(c->device)) return rc;
  Channel& C = c->ch[chl];
  if (C.n != C.nvals)  // CHECK_EQ(key_[ch].size(), val_[ch].size()) kv_vector.h:220
    return fail(PSG_ERR_SIZE, "channel %d: %zu keys but %zu values", chl, C.n, C.nvals);
  if (int rc = chan_words(c, C)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = c->chan_order(C, s)) return rc;
  HIP_TRY(psg::launch_pull(c->dtype, C.d_keys, C.n, C.d_vals, keys_dev, n, out_dev, matched_dev,
                           C.d_dev + 1, c->d_small + kErrUnsorted, s));
  return c->chan_mark(C, s);
}

int psg_darling_update_dev(psg_ctx* c, int chl, int time, const psg_darling_param* p) {
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
  int rc = chan_words(c, C);
  if (rc == PSG_OK) rc = c->flush(A);
  if (rc == PSG_OK) rc = c->chan_order(C, c->stream);  // behind every pull called before
  if (rc == PSG_OK) {
    const psg::DarlingParam P{p->eta, p->lambda, p->kkt_filter_threshold, p->delta_max};
    const hipError_t e = psg::launch_darling_dev(
        (const double*)A.d_out[0], (const double*)A.d_out[1], (double*)C.d_vals, C.d_delta,
        C.d_active, A.lo, A.hi - A.lo, P, A.d_bad, c->d_vio_slots, C.d_dev,
        c->d_small + kErrSkipped, c->stream);
    if (e != hipSuccess) rc = fail(PSG_ERR_DEVICE, "darling update: %s", hipGetErrorString(e));
  }
  if (rc == PSG_OK) rc = c->chan_mark(C, c->stream);
  c->drop(A);
  c->agg.erase(it);
  return rc;
}

int psg_darling_progress(psg_ctx* c, int chl, double lambda, int reset_violation, size_t* nnz_w,
                         double* objv, double* violation, size_t* nnz_active) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  auto it = c->ch.find(chl);
  if (it == c->ch.end() || !it->second.d_active)
    return fail(PSG_ERR_ARG, "channel %d: no Darling state (psg_darling_init)", chl);
  Channel& C = it->second;
  if (C.nvals != C.n || C.dn != C.n)
    return fail(PSG_ERR_SIZE, "channel %d: %zu keys, %zu values, Darling state of %zu", chl,
                C.n, C.nvals, C.dn);
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = chan_words(c, C)) return rc;
  if (int rc = c->ensure_scratch(16 * psg::progress_parts(C.n) + 16)) return rc;
  if (int rc = order_all(c)) return rc;
  unsigned long long* ds = c->d_small;
  HIP_TRY(psg::launch_progress((const double*)C.d_vals, C.n, (unsigned long long*)c->scratch,
                               ds + kProgRes, c->stream));
  HIP_TRY(hipMemsetAsync(ds + kProgActive, 0, 8, c->stream));
  HIP_TRY(psg::launch_popcount(C.d_active, (C.dn + 31) / 32, ds + kProgActive, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small + kErrSkipped, ds + kErrSkipped, 8 * (kProgActive + 1 - kErrSkipped),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small + kProgVio, C.d_dev, 8, hipMemcpyDeviceToHost, c->stream));
  if (reset_violation)  // violation_ = 0 (darling.cc:163-166)
    HIP_TRY(hipMemsetAsync(C.d_dev, 0, 8, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (nnz_w) *nnz_w = (size_t)c->h_small[kProgRes];
  if (objv) {
    double sum;
    memcpy(&sum, c->h_small + kProgRes + 1, 8);
    *objv = lambda * sum;
  }
  if (violation) memcpy(violation, c->h_small + kProgVio, 8);
  if (nnz_active) *nnz_active = (size_t)c->h_small[kProgActive];
  return report_deferred(c);
}

int psg_dev_status(psg_ctx* c) {
  if (!c) return fail(PSG_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> l(c->mu);
  if (int rc = set_dev(c->device)) return rc;
  if (int rc = c->join_copy()) return rc;
  if (int rc = order_all(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->h_small + kErrSkipped, c->d_small + kErrSkipped, 16,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return report_deferred(c);
}

}  // extern "C"
