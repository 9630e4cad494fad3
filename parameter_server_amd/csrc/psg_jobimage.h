// psg_jobimage.h -- the planner of a job table's device image: which kernel
// form a batch of merge jobs takes, where every region of the image lies and
// what is written there.  Pure host code: no HIP call, and the device and
// push pointers it handles are never dereferenced, so it is tested without
// a GPU (tests/cpp/test_jobimage.cc).  JobTable (psg_jobtable.h) owns the
// memory, uploads the image and launches the kernels.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "psg_internal.h"

namespace psg {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct JobSpec {
  const uint64_t* keys;
  uint64_t nslots;
  std::vector<const uint64_t*> pkeys;
  std::vector<const void*> pvals;  // [p*m + i]
  std::vector<uint64_t> pn;
  std::vector<void*> out;
  uint32_t flags;
  // dense job: every non-empty push p is D[dpos[p], dpos[p] + pn[p])
  bool dense = false;
  std::vector<uint64_t> dpos;
};

// per job (host): pushes kept (non-empty) and where their matched counts go
struct JobInfo {
  uint32_t np = 0, ntiles = 0;
  std::vector<uint64_t> pn;          // kept pushes
  std::vector<uint32_t> slot;        // kept push -> index in the caller's push list
  uint32_t ncaller = 0;              // caller's push count (empties included)
  uint32_t* seg = nullptr;
  uint32_t segq = 1;                 // seg stride between pushes
  unsigned long long* fail = nullptr;
  uint32_t kr = 0;                   // cursor form: rounds per push per tile
  uint32_t nch = 0, ch0 = 0;         // cursor forms: chunks, the first of them
  uint32_t nitems = 0, nsplit = 0;   // partition items, splitter items
  bool has_split = false;            // the job has a splitter array
};

// Every region of the image, in image order (byte offsets).  Regions are
// packed back to back, each padded to 256 B except a job's pk, pv, pn and
// out arrays, padded to 64 B; a region the form does not use is empty.
struct JobLayout {
  static constexpr size_t jobs = 0;  // JobDev x njobs
  size_t tiles = 0;                  // TileDesc x ntiles
  size_t index = 0;                  // the resident bucket index: iw u32 per tile
  size_t marked = 0;                 // the index kernel's count of marked tiles
  size_t sitems = 0;                 // splitter items, u32
  size_t items = 0;                  // partition items, u64
  size_t cjobs = 0;                  // cursor form: CursorJob x njobs
  size_t chunks = 0;                 // cursor forms: CursorChunk x nchunks
  // one zeroed region: every job's fail counters, then the boundary words
  size_t zero = 0, bx = 0, zero_end = 0;
  struct Job { size_t pk, pv, pn, out, fail, seg, split, dpos; };
  std::vector<Job> job;
  size_t hstate = 0;                 // hinted plans: one u32 per partition item (kHint*)
  size_t total = 0;
  uint32_t iw = 0;                   // bucket index words per tile
};

struct JobImage {
  // forced forms (JobTable::read_knobs), -1 = chosen
  int knob_part = -1, knob_pack = -1, knob_wide = -1, knob_cursor = -1;

  int dtype = 0, m = 1;
  bool index = false;  // plans: a resident bucket index and splitters, built once
  bool pack = false;   // rounds may hold several pushes
  bool wide = false;   // push groups of 64 in the tile kernel (a job has > 32 pushes)
  bool dense = false;  // every job dense: psg_tile_dense.hip, no partition
  // cursor form (psg_tile_cursor.hip): plans of long pieces, no partition
  // pass; chunks of consecutive tiles, one workgroup each
  bool cursor = false;
  // packed cursor form (psg_tile_packed.hip CUR): short pieces of <= 256
  // pushes, no partition pass either
  bool pcursor = false;
  uint32_t tile = kTileSlots;  // slots per tile
  uint32_t bxs = 32;           // boundary words per chunk boundary (pushes per job at most)
  uint32_t nchunks = 0;
  uint32_t ckr = 3;            // rounds per push per tile (max over the jobs)
  uint32_t ntiles = 0, nitems = 0, nsplit = 0;
  bool all_search = false;  // every job's partition searches (launch_partition xcd)
  // plans (seg lives as long as the plan, zeroed at the build): the search
  // partition tries the cuts the last run left before it searches
  // (psg_partition.hip search_item; off: PSG_NO_HINTS)
  bool hints = false;
  std::vector<JobDev> h;
  std::vector<JobInfo> info;
  JobLayout lay;
  bool use_index() const { return index && !dense; }

  // the shape of the last build whose tile descriptors and work items are
  // on the device (flushes only): a flush of the same shape -- the usual
  // case, the same range of a channel merged time after time -- writes and
  // uploads only the job tables and the pushes' pointers (for a 16.8 M-slot
  // aggregate the descriptors are 1.4 MB)
  std::vector<uint64_t> last_shape, shape;

  // Form and counts: the kernel form, the tile size and per job the JobDev
  // scalars and the JobInfo.  PSG_ERR_ARG past a limit of the image format.
  int plan(const JobSpec* jobs, size_t njobs, int dtype, int m, bool index);
  // Lays the regions out (`iw`: bucket_index_words(tile)).
  void layout(const JobSpec* jobs, uint32_t iw);
  // Builds the key of this shape for an image at device address `base`;
  // true when the last kept shape (keep_shape) equals it.
  bool same_shape(const JobSpec* jobs, const void* base);
  // After the upload: the device now holds this shape.
  void keep_shape();
  // Writes the host image `img` of lay.total bytes for a device copy at
  // `base`; `same`: without the tile descriptors and the items.
  int fill(const JobSpec* jobs, char* img, const void* base, bool same);
};

}  // namespace psg
