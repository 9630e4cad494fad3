// psg_jobtable.h -- job table: the device image of a batch of merge jobs
// (shared by psg_plan and the context's flushes).  The image is planned by
// JobImage (psg_jobimage.h); JobTable owns its memory, uploads it and
// launches the kernels (psg_jobtable.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <vector>

#include "psg_jobimage.h"

namespace psg {

// Marks the jobs whose every non-empty push is a contiguous slice of the
// job's server keys (psg_tile_dense.hip), with each push's start position.
// One synchronous check on the device per plan.
int detect_dense(std::vector<JobSpec>& specs);

struct JobTable : JobImage {
  int device = -1;
  void read_knobs(unsigned flags);  // psg.h PSG_FORM_*, PSG_PART_*, PSG_GROUP*, PSG_NO_ZERO_COPY
  // plans (D fixed for their lifetime): the stream jobs' splitters are
  // written once, at build, and a run launches only the partition proper
  bool split_once = false;
  uint64_t index_bytes = 0, marked_tiles = 0;  // a plan's resident bucket index
  void* blob = nullptr;
  size_t blob_bytes = 0;
  JobDev* d_jobs = nullptr;
  TileDesc* d_tiles = nullptr;
  uint32_t* d_split_items = nullptr;
  uint64_t* d_items = nullptr;
  CursorJob* d_cjobs = nullptr;
  CursorChunk* d_chunks = nullptr;
  uint32_t* d_bx = nullptr;   // chunk boundary words
  uint32_t* d_hstate = nullptr;  // hinted plans: the waves' hint states (psg_internal.h kHint*)
  void* d_zero = nullptr;     // fail counters of every job + boundary words: zeroed per run
  size_t zero_bytes = 0;
  // pinned host images of the blob, used alternately: a build fills one
  // while the previous build's copy may still be in flight
  char* himg[2] = {nullptr, nullptr};
  const void* himg_dev[2] = {nullptr, nullptr};  // their device-visible addresses
  bool zero_copy = true;  // the image moves by the zero-copy kernel, not a DMA copy
  size_t himg_cap[2] = {0, 0};
  hipEvent_t himg_ev[2] = {nullptr, nullptr};
  int himg_cur = 0;

  void release();
  // Builds (or rebuilds, reusing the allocation when it fits) the device
  // image (JobLayout).  The image is copied on stream `strm`, without a host
  // wait when `async`; work enqueued on `strm` afterwards sees it.
  // `index`: give the tile kernel's tiles a resident bucket table (built
  // here, once, from D: plans, whose D is fixed for their lifetime)
  int build(int dev, int dtype, int m, const std::vector<JobSpec>& jobs,
            hipStream_t strm = nullptr, bool async = false, bool index = false);
  int run_stage(int stage, hipStream_t s) const;
  int run(hipStream_t s) const;
  // matched[p] per caller push (empty pushes 0): covered elements minus
  // match failures; the stream must be idle.
  int matched(std::vector<uint64_t>& out) const;

 private:
  void release_blob();
  // the blob and the host image `ib`, each at least lay.total bytes
  int ensure_memory(int ib, hipStream_t strm, bool async);
  int upload(int ib, bool same, hipStream_t strm);
};

}  // namespace psg
