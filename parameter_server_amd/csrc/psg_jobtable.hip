// psg_jobtable.hip -- the HIP side of a job table (psg_jobtable.h): the
// image's memory, its upload, the launches that read it.
#include "psg_jobtable.h"

#include <utility>

#include "psg_host.h"

namespace psg {

int detect_dense(std::vector<JobSpec>& specs) {
  std::vector<DenseCheck> hc;
  std::vector<std::pair<size_t, size_t>> at;  // (job, push) of each check
  std::vector<uint64_t> items;
  for (size_t j = 0; j < specs.size(); ++j) {
    const JobSpec& s = specs[j];
    if (s.nslots == 0) continue;
    for (size_t p = 0; p < s.pn.size(); ++p) {
      if (s.pn[p] == 0) continue;
      if (s.pn[p] > s.nslots) goto next_job;  // cannot be a slice
      at.emplace_back(j, p);
      hc.push_back(DenseCheck{s.pkeys[p], s.pn[p], s.keys, s.nslots, nullptr});
    }
  next_job:;
  }
  if (hc.empty()) return PSG_OK;
  for (size_t c = 0; c < hc.size(); ++c)
    for (uint64_t q = 0; q * 4096 < hc[c].n; ++q) items.push_back((uint64_t)c << 32 | q);
  const size_t ob = align_up(16 * hc.size(), 256), cb = align_up(sizeof(DenseCheck) * hc.size(), 256);
  char* tmp = nullptr;
  HIP_TRY(hipMalloc((void**)&tmp, ob + cb + 8 * items.size()));
  unsigned long long* outs = (unsigned long long*)tmp;
  for (size_t c = 0; c < hc.size(); ++c) hc[c].out = outs + 2 * c;
  std::vector<unsigned long long> ho(2 * hc.size());
  hipError_t e = hipMemset(outs, 0, 16 * hc.size());
  if (e == hipSuccess) e = hipMemcpy(tmp + ob, hc.data(), sizeof(DenseCheck) * hc.size(),
                                     hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(tmp + ob + cb, items.data(), 8 * items.size(),
                                     hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = launch_dense_check((const DenseCheck*)(tmp + ob), (uint32_t)hc.size(),
                           (const uint64_t*)(tmp + ob + cb), items.size(), nullptr);
  if (e == hipSuccess) e = hipMemcpy(ho.data(), outs, 16 * hc.size(), hipMemcpyDeviceToHost);
  (void)hipFree(tmp);
  if (e != hipSuccess) return fail(PSG_ERR_DEVICE, "dense check: %s", hipGetErrorString(e));
  std::vector<int> ok(specs.size(), -1);  // -1 unchecked, 1 dense so far, 0 not
  for (size_t c = 0; c < hc.size(); ++c) {
    const size_t j = at[c].first;
    if (ok[j] < 0) {
      ok[j] = 1;
      specs[j].dpos.assign(specs[j].pn.size(), 0);
    }
    if (ho[2 * c + 1]) ok[j] = 0;
    specs[j].dpos[at[c].second] = ho[2 * c];
  }
  for (size_t j = 0; j < specs.size(); ++j) {
    // every non-empty push was checked (none skipped by the size test)
    size_t nonempty = 0, checked = 0;
    for (uint64_t n : specs[j].pn) nonempty += n != 0;
    for (const auto& a : at) checked += a.first == j;
    specs[j].dense = ok[j] == 1 && checked == nonempty && nonempty > 0;
    if (!specs[j].dense) specs[j].dpos.clear();
  }
  return PSG_OK;
}

void JobTable::read_knobs(unsigned f) {
  knob_cursor = (f & PSG_FORM_CURSOR) ? 1 : (f & PSG_NO_CURSOR) ? 0 : -1;
  knob_part = (f & PSG_PART_SEARCH) ? (int)kSearch : (f & PSG_PART_STREAM) ? (int)kStream : -1;
  knob_pack = (f & PSG_FORM_PACKED) ? 1 : (f & PSG_FORM_UNIFORM) ? 0 : -1;
  knob_wide = (f & PSG_GROUP64) ? 1 : (f & PSG_GROUP32) ? 0 : -1;
  zero_copy = !(f & PSG_NO_ZERO_COPY);
}

void JobTable::release_blob() {
  if (blob) (void)hipFree(blob);
  blob = nullptr;
  blob_bytes = 0;
  last_shape.clear();
}

void JobTable::release() {
  release_blob();
  for (int i = 0; i < 2; ++i) {
    if (himg_ev[i]) (void)hipEventSynchronize(himg_ev[i]);
    if (himg_ev[i]) (void)hipEventDestroy(himg_ev[i]);
    if (himg[i]) (void)hipHostFree(himg[i]);
    himg[i] = nullptr;
    himg_dev[i] = nullptr;
    himg_ev[i] = nullptr;
    himg_cap[i] = 0;
  }
}

int JobTable::ensure_memory(int ib, hipStream_t strm, bool async) {
  const size_t need = lay.total;
  if (need > blob_bytes) {
    if (async) HIP_TRY(hipStreamSynchronize(strm));  // the old blob may be in use
    release_blob();
    HIP_TRY(hipMalloc(&blob, need));
    blob_bytes = need;
  }
  // the copy of the build before last, out of this host image
  if (himg_ev[ib]) HIP_TRY(hipEventSynchronize(himg_ev[ib]));
  else HIP_TRY(hipEventCreateWithFlags(&himg_ev[ib], hipEventDisableTiming));
  if (need > himg_cap[ib]) {
    if (himg[ib]) HIP_TRY(hipHostFree(himg[ib]));
    himg[ib] = nullptr;
    himg_cap[ib] = 0;
    HIP_TRY(hipHostMalloc((void**)&himg[ib], need));
    himg_cap[ib] = need;
    himg_dev[ib] = nullptr;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, himg[ib], 0) == hipSuccess) himg_dev[ib] = dp;
    else (void)hipGetLastError();
  }
  return PSG_OK;
}

// the image is small: a DMA copy's fixed cost exceeds its transfer time.
// Same shape: the job tables and the regions after the items only
int JobTable::upload(int ib, bool same, hipStream_t strm) {
  const char* img = himg[ib];
  char* base = (char*)blob;
  const size_t total = lay.total, head = lay.tiles, tail = lay.zero;
  const bool zc_ok = zero_copy && himg_dev[ib] && (((uintptr_t)himg_dev[ib] | (uintptr_t)blob) & 15u) == 0;
  if (same && zc_ok) {
    HostCopyBatch cb;
    cb.n = 2;
    cb.d[0] = HostCopyDesc{himg_dev[ib], blob, (uint64_t)head};
    cb.d[1] = HostCopyDesc{(const char*)himg_dev[ib] + tail, base + tail, (uint64_t)(total - tail)};
    HIP_TRY(launch_host_copy_batch(cb, strm));
  } else if (same) {
    HIP_TRY(hipMemcpyAsync(blob, img, head, hipMemcpyHostToDevice, strm));
    HIP_TRY(hipMemcpyAsync(base + tail, img + tail, total - tail, hipMemcpyHostToDevice, strm));
  } else if (zc_ok) {
    HIP_TRY(launch_host_copy(blob, himg_dev[ib], total, strm));
  } else {
    HIP_TRY(hipMemcpyAsync(blob, img, total, hipMemcpyHostToDevice, strm));
  }
  return PSG_OK;
}

int JobTable::build(int dev, int dt, int mm, const std::vector<JobSpec>& jobs, hipStream_t strm,
                    bool async, bool idx) {
  device = dev;
  if (int rc = plan(jobs.data(), jobs.size(), dt, mm, idx)) return rc;
  layout(jobs.data(), bucket_index_words(tile));
  const int ib = himg_cur;
  himg_cur ^= 1;
  if (int rc = ensure_memory(ib, strm, async)) return rc;
  const bool same = same_shape(jobs.data(), blob);
  if (int rc = fill(jobs.data(), himg[ib], blob, same)) return rc;
  char* base = (char*)blob;
  const bool chunked = cursor || pcursor;
  d_jobs = (JobDev*)blob;
  d_tiles = (TileDesc*)(base + lay.tiles);
  d_split_items = (uint32_t*)(base + lay.sitems);
  d_items = (uint64_t*)(base + lay.items);
  d_cjobs = cursor ? (CursorJob*)(base + lay.cjobs) : nullptr;
  d_chunks = chunked ? (CursorChunk*)(base + lay.chunks) : nullptr;
  d_bx = chunked ? (uint32_t*)(base + lay.bx) : nullptr;
  d_hstate = hints && nitems ? (uint32_t*)(base + lay.hstate) : nullptr;
  d_zero = base + lay.zero;
  zero_bytes = lay.zero_end - lay.zero;
  if (int rc = upload(ib, same, strm)) return rc;
  keep_shape();
  HIP_TRY(hipEventRecord(himg_ev[ib], strm));
  index_bytes = 0;
  marked_tiles = 0;
  unsigned long long* d_marked = (unsigned long long*)(base + lay.marked);
  if (use_index())
    HIP_TRY(launch_bucket_index(d_tiles, ntiles, tile, (uint32_t*)(base + lay.index), d_marked,
                                strm));
  split_once = index && nsplit > 0 && !dense && !chunked;
  if (split_once)  // the splitter pass alone (it also clears the fail counters once)
    HIP_TRY(launch_partition(d_jobs, d_split_items, nsplit, nullptr, 0, strm));
  if (!async) HIP_TRY(hipStreamSynchronize(strm));
  if (use_index()) {  // plans only (built synchronously)
    index_bytes = 4 * (uint64_t)lay.iw * ntiles;
    if (ntiles) {
      HIP_TRY(hipMemcpyAsync(&marked_tiles, d_marked, 8, hipMemcpyDeviceToHost, strm));
      HIP_TRY(hipStreamSynchronize(strm));
    }
  }
  return PSG_OK;
}

int JobTable::run_stage(int stage, hipStream_t s) const {
  if (h.empty()) return PSG_OK;
  if (stage == 0) {
    if (cursor || pcursor)  // fail counters, boundaries
      HIP_TRY(hipMemsetAsync(d_zero, 0, zero_bytes, s));
    else if (!dense)
      HIP_TRY(launch_partition(d_jobs, d_split_items, split_once ? 0u : nsplit, d_items, nitems, s,
                               all_search, d_hstate));
  } else if (cursor)
    HIP_TRY(launch_aggregate_cursor(dtype, m, (int)ckr, d_cjobs, d_chunks, nchunks, d_bx, s));
  else if (dense)
    HIP_TRY(launch_aggregate_dense(dtype, m, d_tiles, ntiles, s));
  else if (pack)
    HIP_TRY(launch_aggregate_tile_packed(dtype, m, d_tiles, ntiles, s,
                                         pcursor ? d_chunks : nullptr, nchunks, d_bx));
  else
    HIP_TRY(launch_aggregate_tile(dtype, m, d_tiles, ntiles, wide ? 1 : 0, s));
  return PSG_OK;
}

int JobTable::run(hipStream_t s) const {
  if (int rc = run_stage(0, s)) return rc;
  return run_stage(1, s);
}

int JobTable::matched(std::vector<uint64_t>& out) const {
  out.clear();
  for (size_t j = 0; j < h.size(); ++j) {
    const JobInfo& I = info[j];
    std::vector<uint64_t> mt(I.ncaller, 0);
    const uint32_t np = I.np, nt = I.ntiles;
    if (np && nt) {
      std::vector<unsigned long long> f(np);
      std::vector<uint32_t> first(np), last(np);
      const size_t pitch = 4 * (size_t)I.segq;
      const size_t segb = I.segq == 1 ? np : 1;  // tile-major / push-major
      HIP_TRY(hipMemcpy(f.data(), I.fail, 8 * np, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy2D(first.data(), 4, I.seg, pitch, 4, np, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy2D(last.data(), 4, I.seg + (size_t)nt * segb, pitch, 4, np,
                          hipMemcpyDeviceToHost));
      // cursor form: a chunk boundary where the chunks' cursors disagree
      // (start != the previous chunk's end) means an unsorted push
      std::vector<uint32_t> bxw;
      const bool cur = cursor || pcursor;
      if (cur && I.nch > 1) {
        bxw.resize((size_t)bxs * (I.nch - 1));
        HIP_TRY(hipMemcpy(bxw.data(), d_bx + (size_t)bxs * (I.ch0 + 1), 4 * bxw.size(),
                          hipMemcpyDeviceToHost));
      }
      for (uint32_t p = 0; p < np; ++p) {
        const uint64_t covered = last[p] >= first[p] ? (uint64_t)(last[p] - first[p]) : 0;
        uint64_t v = covered >= f[p] ? covered - f[p] : 0;
        bool torn = false;
        for (size_t k = 0; k + 1 < I.nch && cur; ++k) torn |= bxw[(size_t)bxs * k + p] != 0;
        if (torn && v >= I.pn[p]) v = I.pn[p] - 1;
        mt[I.slot[p]] = v;
      }
    }
    out.insert(out.end(), mt.begin(), mt.end());
  }
  return PSG_OK;
}

}  // namespace psg
