// psg_plan.hip -- the plan API (a device-resident batch of merge jobs run
// any number of times) and the stateless device helpers of the C ABI
// (include/psg.h): none of them needs a context.
#include "psg_ctx.h"

// ==========================================================================
// plan API (device-resident batch)
// ==========================================================================
struct psg_plan {
  JobTable table;
  hipStream_t last = nullptr;
  uint64_t bytes = 0, kv = 0;
};

extern "C" {

int psg_plan_max_push(void) { return psg::kMaxPush; }

// ---------------------------------------------------------------- plans --
int psg_plan_create(int device, int dtype, int m, unsigned flags,
                    const psg_merge_job* jobs, int njobs, psg_plan** out) {
  if (!out || (njobs > 0 && !jobs)) return fail(PSG_ERR_ARG, "null argument");
  if (dtype != PSG_F32 && dtype != PSG_F64) return fail(PSG_ERR_ARG, "dtype %d", dtype);
  if (m < 1 || m > PSG_MAX_VALUE_ARRAYS) return fail(PSG_ERR_ARG, "m=%d", m);
  if (int rc = set_dev(device)) return rc;
  std::vector<JobSpec> specs(njobs);
  uint64_t bytes = 0, kv = 0;
  const uint64_t sv = vsize(dtype);
  for (int j = 0; j < njobs; ++j) {
    const psg_merge_job& J = jobs[j];
    if (J.npush < 0 || (J.npush > 0 && (!J.push_keys || !J.push_vals || !J.push_n)) ||
        !J.out || (J.nslots > 0 && !J.keys))
      return fail(PSG_ERR_ARG, "job %d: null pointer", j);
    JobSpec& s = specs[j];
    s.keys = J.keys;
    s.nslots = J.nslots;
    s.flags = (flags & PSG_PARALLEL_MATCH) ? psg::kFlagParallel : 0u;
    for (int p = 0; p < J.npush; ++p) {
      s.pkeys.push_back(J.push_keys[p]);
      for (int i = 0; i < m; ++i) s.pvals.push_back(J.push_vals[(size_t)p * m + i]);
      s.pn.push_back(J.push_n[p]);
      bytes += J.push_n[p] * (8 + m * sv);
      kv += J.push_n[p];
    }
    for (int i = 0; i < m; ++i) s.out.push_back(J.out[i]);
    bytes += J.nslots * (8 + m * sv);
  }
  // the dense kernel reads no push keys: only for keys the caller fixed
  // (PSG_STATIC_KEYS, psg.h); otherwise every run re-checks them
  if ((flags & PSG_STATIC_KEYS) && !(flags & PSG_NO_DENSE))
    if (int rc = detect_dense(specs)) return rc;
  psg_plan* p = new psg_plan();
  p->table.read_knobs(flags);
  p->table.hints = !(flags & PSG_NO_HINTS);
  int rc = p->table.build(device, dtype, m, specs, nullptr, false, !(flags & PSG_NO_INDEX));
  if (rc) {
    p->table.release();
    delete p;
    return rc;
  }
  p->bytes = bytes;
  p->kv = kv;
  *out = p;
  return PSG_OK;
}

int psg_plan_run(psg_plan* plan, void* stream) {
  if (!plan) return fail(PSG_ERR_ARG, "null plan");
  plan->last = (hipStream_t)stream;
  return plan->table.run((hipStream_t)stream);
}

int psg_plan_run_stage(psg_plan* plan, int stage, void* stream) {
  if (!plan || stage < 0 || stage > 1) return fail(PSG_ERR_ARG, "bad plan/stage");
  plan->last = (hipStream_t)stream;
  return plan->table.run_stage(stage, (hipStream_t)stream);
}

int psg_plan_matched(psg_plan* plan, uint64_t* matched) {
  if (!plan || !matched) return fail(PSG_ERR_ARG, "null argument");
  if (int rc = set_dev(plan->table.device)) return rc;
  HIP_TRY(hipStreamSynchronize(plan->last));
  std::vector<uint64_t> mt;
  if (int rc = plan->table.matched(mt)) return rc;
  std::copy(mt.begin(), mt.end(), matched);
  return PSG_OK;
}

int psg_plan_form(psg_plan* plan, int* form) {
  if (!plan || !form) return fail(PSG_ERR_ARG, "null argument");
  const JobTable& T = plan->table;
  *form = T.cursor ? PSG_KERNEL_CURSOR
          : T.pcursor ? PSG_KERNEL_PACKED_CURSOR
          : T.dense ? PSG_KERNEL_DENSE
          : T.pack  ? PSG_KERNEL_PACKED
          : T.wide  ? PSG_KERNEL_TILE64
                    : PSG_KERNEL_TILE;
  return PSG_OK;
}

int psg_plan_index_info(psg_plan* plan, uint64_t* index_bytes, uint64_t* marked_tiles) {
  if (!plan) return fail(PSG_ERR_ARG, "null plan");
  if (index_bytes) *index_bytes = plan->table.index_bytes;
  if (marked_tiles) *marked_tiles = plan->table.marked_tiles;
  return PSG_OK;
}

int psg_plan_hint_state(psg_plan* plan, uint64_t counts[4]) {
  if (!plan || !counts) return fail(PSG_ERR_ARG, "null argument");
  const JobTable& T = plan->table;
  for (int i = 0; i < 4; ++i) counts[i] = 0;
  if (!T.d_hstate) return PSG_OK;
  if (int rc = set_dev(T.device)) return rc;
  HIP_TRY(hipStreamSynchronize(plan->last));
  std::vector<uint32_t> st(T.nitems);
  HIP_TRY(hipMemcpy(st.data(), T.d_hstate, 4 * (size_t)T.nitems, hipMemcpyDeviceToHost));
  size_t i = 0;  // a job's items are consecutive
  for (size_t j = 0; j < T.h.size(); ++j)
    for (uint32_t k = 0; k < T.info[j].nitems; ++k, ++i)
      if (T.h[j].mode == psg::kSearch) counts[st[i] & 3u]++;
  return PSG_OK;
}

int psg_plan_bytes(psg_plan* plan, uint64_t* bytes, uint64_t* kv) {
  if (!plan) return fail(PSG_ERR_ARG, "null plan");
  if (bytes) *bytes = plan->bytes;
  if (kv) *kv = plan->kv;
  return PSG_OK;
}

int psg_plan_destroy(psg_plan* plan) {
  if (!plan) return PSG_OK;
  (void)hipSetDevice(plan->table.device);
  plan->table.release();
  delete plan;
  return PSG_OK;
}

// -------------------------------------------------------- device helpers --
int psg_gather_dev(int dtype, const uint64_t* dkeys, uint64_t nd,
                   const void* dvals, const uint64_t* req, uint64_t nreq,
                   void* out, unsigned long long* matched, void* stream) {
  if (dtype != PSG_F32 && dtype != PSG_F64) return fail(PSG_ERR_ARG, "dtype");
  HIP_TRY(psg::launch_gather(dtype, dkeys, nd, dvals, req, nreq, out, matched,
                             (hipStream_t)stream));
  return PSG_OK;
}

int psg_key_union_dev(const uint64_t* a, uint64_t na, const uint64_t* b,
                      uint64_t nb, uint64_t* out, uint64_t* nout, void* stream) {
  if (!out || !nout || (na && !a) || (nb && !b)) return fail(PSG_ERR_ARG, "null");
  if (na + nb >= (1ull << 32)) return fail(PSG_ERR_ARG, "na + nb >= 2^32");
  hipStream_t s = (hipStream_t)stream;
  std::vector<const uint64_t*> pk;
  std::vector<uint64_t> pn;
  if (na) { pk.push_back(a); pn.push_back(na); }
  if (nb) { pk.push_back(b); pn.push_back(nb); }
  void* scratch = nullptr;
  HIP_TRY(hipMalloc(&scratch, psg::nway_scratch_bytes((uint32_t)pk.size(), pn.data())));
  unsigned long long* d_bad = nullptr;
  unsigned long long h[2] = {0, 0};
  hipError_t e = psg::nway_union_enqueue((uint32_t)pk.size(), pk.data(), pn.data(), out, scratch,
                                         &d_bad, s);
  if (e == hipSuccess) e = hipMemcpyAsync(h, d_bad, 16, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(scratch);
  if (e != hipSuccess) return fail(PSG_ERR_DEVICE, "key union: %s", hipGetErrorString(e));
  // high bits: tile overflow (1 << 32) / look-back timeout (1 << 40) of the
  // N-way kernels: a device fault and not an order violation, unless an
  // input is not strictly increasing (only then can a tile overflow)
  if (h[0] >> 32) {
    bool dis = false;
    HIP_TRY(psg::nway_disordered((uint32_t)pk.size(), pk.data(), pn.data(), s, &dis));
    if (!dis) return fail(PSG_ERR_DEVICE, "key union: device fault (%llx)", h[0]);
    return fail(PSG_ERR_UNSORTED, "an input is not strictly increasing (%llx)", h[0]);
  }
  if (h[0]) return fail(PSG_ERR_UNSORTED, "%llu order violations", h[0]);
  *nout = h[1];
  return PSG_OK;
}

int psg_shard_bounds(size_t n, uint64_t* bounds) {
  if (n == 0 || !bounds) return fail(PSG_ERR_ARG, "n == 0");
  // Range<uint64>::all() = [0, 2^64-1)  (range.h:75-78); evenDivide (:85-98)
  const uint64_t b = 0, e = ~0ull;
  const long double itv = (long double)(e - b) / (long double)n;
  for (size_t i = 0; i < n; ++i) bounds[i] = (uint64_t)(b + itv * (long double)i);
  bounds[n] = e;
  return PSG_OK;
}

int psg_slice_dev(const uint64_t* keys, uint64_t n, uint64_t kb, uint64_t ke,
                  const uint64_t* sep, int nsep, uint64_t* pos, void* stream) {
  if (nsep < 0 || (nsep > 0 && (!sep || !pos))) return fail(PSG_ERR_ARG, "null");
  HIP_TRY(psg::launch_slice(keys, n, kb, ke, sep, nsep, pos, (hipStream_t)stream));
  return PSG_OK;
}

int psg_crc32c_dev(const void* data, const uint64_t* off, uint64_t nseg, uint64_t max_len,
                   const uint32_t* init, uint32_t* out, void* stream) {
  if (nseg == 0) return PSG_OK;
  if (!data || !off || !out) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(psg::launch_crc32c((const uint8_t*)data, off, nseg, max_len, init, out,
                             (hipStream_t)stream));
  return PSG_OK;
}

int psg_snappy_uncompress_dev(const uint8_t* src, const uint64_t* soff, uint64_t nmsg,
                              uint8_t* dst, const uint64_t* doff, int32_t* status,
                              void* stream) {
  if (nmsg == 0) return PSG_OK;
  if (!src || !soff || !dst || !doff || !status) return fail(PSG_ERR_ARG, "null argument");
  // the deferred-literal list, stream-ordered (freed behind the kernels)
  hipStream_t st = (hipStream_t)stream;
  void* scratch = nullptr;
  HIP_TRY(hipMallocAsync(&scratch, psg::snappy_scratch_bytes(nmsg), st));
  const hipError_t e =
      psg::launch_snappy(src, soff, nmsg, dst, doff, nullptr, status, scratch, st, nullptr);
  HIP_TRY(hipFreeAsync(scratch, st));
  HIP_TRY(e);
  return PSG_OK;
}

size_t psg_snappy_compress_scratch_bytes(size_t total_src_bytes, uint64_t nparts) {
  return psg::snappy_compress_scratch_bytes(total_src_bytes, nparts);
}

int psg_snappy_compress_dev(const uint8_t* src, const uint64_t* soff, uint64_t nparts,
                            uint8_t* dst, const uint64_t* doff, uint64_t* clen, void* scratch,
                            void* stream) {
  if (nparts == 0) return PSG_OK;
  if (!src || !soff || !dst || !doff || !clen || !scratch)
    return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(psg::launch_snappy_compress(src, soff, nparts, dst, doff, clen, scratch,
                                      (hipStream_t)stream));
  return PSG_OK;
}

int psg_snappy_uncompressed_length(const void* src, size_t n, size_t* len) {
  if (!len || (n && !src)) return fail(PSG_ERR_ARG, "null argument");
  // the preamble: a little-endian base-128 varint of at most 32 bits
  const uint8_t* p = (const uint8_t*)src;
  uint64_t v = 0;
  for (size_t i = 0; i < n && i < 5; ++i) {
    v |= (uint64_t)(p[i] & 0x7f) << (7 * i);
    if (!(p[i] & 0x80)) {
      if (v > 0xffffffffull) break;
      *len = (size_t)v;
      return PSG_OK;
    }
  }
  return fail(PSG_ERR_ARG, "snappy: bad length preamble");
}

}  // extern "C"
