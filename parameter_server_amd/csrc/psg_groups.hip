// psg_groups.hip -- the feature groups of a loaded minibatch (DESIGN.md
// 4.11b): ExampleParser::toProto's bookkeeping and info()
// (src/data/example_parser.cc:38-82) over the entries' slot ids, and
// SlotReader's per-slot storage (src/data/slot_reader.cc:146-166,234-290) as
// one resident minibatch per group.
//
//  (1) widen_kernel: the 16-bit slot ids as the sort's 64-bit keys; an id
//      outside [1, 4095] marks its row bad.
//  (2) the stable radix sort of psg_sort.h over (slot, position), on the
//      digits in which the ids differ (at most two): every slot's entries
//      become one segment of the sorted pairs, in their original order.
//  (3) the run heads of psg_sort.h over the sorted ids: the slots present in
//      ascending order, each one's segment, the segment of every pair.
//  (4) stat_kernel, one lane per sorted pair: two neighbours of one slot and
//      one row must be neighbours in the row too, or the row is bad (the
//      slot occurs in two separate runs); a pair that is the first of its
//      slot in its row counts one example; the keys' minimum and the maximum
//      of key + 1.  A wave whose pairs share one slot folds them first.
//  (5) the host reads the two control words and the statistics: one wait.
// psg_mb_group_extract gathers one segment: index / value by the segment's
// positions, offset_g[r] = the segment's positions below offset[r].
// Integer atomics only (min, max, add): the same input gives the same bytes
// on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <new>

#include "../../include/psg.h"
#include "psg_host.h"
#include "psg_minibatch.h"
#include "psg_sort.h"

namespace psg {
namespace {

constexpr uint32_t kSlotMax = 4096;  // kSlotIDmax: the ids are 1 .. kSlotMax - 1
constexpr uint32_t kNoRow = 0xffffffffu;
constexpr size_t kHeadBytes = 16;  // control words: [0] the slots present, [1] the smallest bad row

struct SlotStat {  // one slot present in the load
  unsigned long long min_key, max_key;
  uint32_t nnz_ex, start, end, id;
};

__global__ __launch_bounds__(256) void widen_kernel(const uint16_t* __restrict__ slot,
                                                    const uint32_t* __restrict__ row_of,
                                                    uint32_t n, uint64_t* __restrict__ key,
                                                    uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = slot[i];
  key[i] = s;
  if (s < 1 || s >= kSlotMax) atomicMin(bad, row_of[i]);
}

__global__ __launch_bounds__(256) void stat_init_kernel(SlotStat* __restrict__ st, uint32_t cap) {
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g < cap) st[g] = SlotStat{~0ull, 0ull, 0u, 0u, 0u, 0u};
}

__global__ __launch_bounds__(256) void stat_kernel(
    const uint64_t* __restrict__ skey, const uint32_t* __restrict__ spos,
    const uint32_t* __restrict__ run_of, const uint32_t* __restrict__ run_start,
    const uint32_t* __restrict__ row_of, const uint64_t* __restrict__ index, uint32_t n,
    uint32_t cap, SlotStat* __restrict__ st, uint32_t* __restrict__ bad) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool valid = j < n;
  uint32_t g = 0, ex = 0;
  unsigned long long lo = ~0ull, hi = 0ull;
  if (valid) {
    g = run_of[j];
    const uint32_t p = spos[j], r = row_of[p];
    const bool head = j == 0 || run_of[j - 1] != g;
    bool row_head = head;
    if (!head) {
      const uint32_t q = spos[j - 1];
      row_head = row_of[q] != r;
      if (!row_head && q + 1 != p) atomicMin(bad, r);  // two runs of the slot in row r
    }
    ex = row_head ? 1u : 0u;
    lo = index[p];
    hi = lo + 1ull;  // as written: key 2^64 - 1 gives 0
    if (head && g < cap) {
      st[g].start = (uint32_t)j;
      st[g].end = run_start[g + 1];
      st[g].id = (uint32_t)skey[j];
    }
  }
  // every lane of the wave comes here
  const uint32_t g0 = __shfl(g, 0, 64);
  const bool uniform = __ballot(valid && g != g0) == 0 && __ballot(valid) != 0;
  if (uniform) {
    for (int s = 32; s >= 1; s >>= 1) {
      const unsigned long long l2 = __shfl_xor(lo, s, 64), h2 = __shfl_xor(hi, s, 64);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
      ex += __shfl_xor(ex, s, 64);
    }
    if (lane == 0 && g0 < cap) {  // lane 0 is valid: the valid lanes are the wave's first
      atomicMin(&st[g0].min_key, lo);
      atomicMax(&st[g0].max_key, hi);
      if (ex) atomicAdd(&st[g0].nnz_ex, ex);
    }
  } else if (valid && g < cap) {
    atomicMin(&st[g].min_key, lo);
    atomicMax(&st[g].max_key, hi);
    if (ex) atomicAdd(&st[g].nnz_ex, ex);
  }
}

// the group's entries in their original order
__global__ __launch_bounds__(256) void group_gather_kernel(const uint32_t* __restrict__ seg,
                                                           uint32_t len,
                                                           const uint64_t* __restrict__ index,
                                                           const double* __restrict__ value,
                                                           uint64_t* __restrict__ out_index,
                                                           double* __restrict__ out_value) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= len) return;
  const uint32_t p = seg[j];
  out_index[j] = index[p];
  if (value) out_value[j] = value[p];
}

// offset_g[r] = the group's entries before offset[r]
__global__ __launch_bounds__(256) void group_offset_kernel(const uint64_t* __restrict__ offset,
                                                           uint32_t rows,
                                                           const uint32_t* __restrict__ seg,
                                                           uint32_t len,
                                                           uint64_t* __restrict__ out_offset) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r > rows) return;
  out_offset[r] = lower_bound<uint32_t>(seg, len, (uint32_t)offset[r]);
}

}  // namespace
}  // namespace psg

using psg::fail;

extern "C" {

int psg_mb_set_slots(psg_minibatch* mb, const uint16_t* slot, size_t n) {
  using namespace psg;
  if (!mb || (n && !slot)) return fail(PSG_ERR_ARG, "null argument");
  if (mb->state != S_LOADED)
    return fail(PSG_ERR_ARG, "psg_mb_set_slots needs a loaded minibatch, before psg_mb_uniq");
  if (n != mb->nnz) return fail(PSG_ERR_SIZE, "%zu slot ids for %zu entries", n, mb->nnz);
  HIP_TRY(hipSetDevice(mb->device));
  mb->has_slots = mb->groups_ok = false;
  if (int rc = mb->need(B_SLOT, 2 * n)) return rc;
  if (int rc = mb->settle()) return rc;
  uint16_t o = 0, a = 0xffffu;
  for (size_t i = 0; i < n; ++i) {
    o |= slot[i];
    a &= slot[i];
  }
  if (n) HIP_TRY(hipMemcpy(mb->b[B_SLOT].p, slot, 2 * n, hipMemcpyHostToDevice));
  mb->slot_differ = n ? (uint64_t)(uint16_t)(o ^ a) : 0;
  mb->has_slots = true;
  return PSG_OK;
}

int psg_mb_groups(psg_minibatch* mb, psg_slot_info* info, size_t cap, size_t* n_out,
                  int64_t* bad_row) {
  using namespace psg;
  if (!mb || !n_out || !bad_row) return fail(PSG_ERR_ARG, "null argument");
  *n_out = 0;
  *bad_row = -1;
  if (mb->state != S_LOADED || !mb->has_slots)
    return fail(PSG_ERR_ARG, "psg_mb_groups needs psg_mb_set_slots, before psg_mb_uniq");
  HIP_TRY(hipSetDevice(mb->device));
  mb->groups_ok = false;
  mb->groups.clear();
  const uint32_t n = (uint32_t)mb->nnz;
  // a 16-bit id: at most 2^16 slots, whatever the caller's array holds
  const uint32_t scap = std::min<uint32_t>(n, 65536u);
  std::vector<SlotStat> h_stat;
  uint32_t head[4] = {0, kNoRow, 0, 0};
  if (n) {
    if (int rc = mb->need(B_GRP, kHeadBytes + sizeof(SlotStat) * (size_t)scap)) return rc;
    hipStream_t s = mb->stream;
    if (int rc = mb->order(s)) return rc;
    uint32_t* words = mb->at<uint32_t>(B_GRP);
    SlotStat* st = (SlotStat*)((char*)mb->b[B_GRP].p + kHeadBytes);
    HIP_TRY(hipMemsetAsync(words, 0xff, kHeadBytes, s));
    uint64_t* key = mb->at<uint64_t>(B_KEY_B);
    LAUNCH(widen_kernel, blocks_of(n, 256), s, mb->at<uint16_t>(B_SLOT),
           mb->at<uint32_t>(B_ROW_OF), n, key, words + 1);
    const SortBuffers sb{mb->at<uint64_t>(B_KEY_A), key, mb->at<uint32_t>(B_POS_A),
                         mb->at<uint32_t>(B_POS_B), mb->at<uint32_t>(B_COUNTS), mb->d_dtotal()};
    if (int rc = enqueue_radix_sort(key, n, mb->slot_differ, sb, &mb->skey, &mb->spos, s)) return rc;
    const HeadFlag f{mb->skey};
    const HeadEmit e{mb->skey, mb->at<uint64_t>(B_UNIQ_KEY), mb->at<uint32_t>(B_RUN_START),
                     mb->at<uint32_t>(B_RUN_OF)};
    enqueue_flag_scan(f, e, n, mb->at<uint32_t>(B_TILE_SUM), words, s);
    LAUNCH(stat_init_kernel, blocks_of(scap, 256), s, st, scap);
    LAUNCH(stat_kernel, blocks_of(n, 256), s, mb->skey, mb->spos, mb->at<uint32_t>(B_RUN_OF),
           mb->at<uint32_t>(B_RUN_START), mb->at<uint32_t>(B_ROW_OF), mb->at<uint64_t>(B_INDEX), n,
           scap, st, words + 1);
    if (int rc = launched("groups")) return rc;
    const uint32_t take = std::min<uint32_t>(scap, kSlotMax);  // more slots than ids: a bad row
    try {
      h_stat.resize(take);
    } catch (const std::bad_alloc&) {
      return fail(PSG_ERR_OOM, "host allocation");
    }
    HIP_TRY(hipMemcpyAsync(head, words, kHeadBytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_stat.data(), st, sizeof(SlotStat) * (size_t)take,
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // the slots and the verdict
    mb->last_s = nullptr;
    if (head[0] == 0 || head[0] > scap)
      return fail(PSG_ERR_DEVICE, "%u slots of %u entries", head[0], n);
  }
  if (head[1] != kNoRow) {
    *bad_row = head[1];
    return fail(PSG_ERR_ARG,
                "row %u holds a slot id outside [1, 4095] or one slot id in two separate runs",
                head[1]);
  }
  const size_t ng = head[0];  // <= 4095: every id is in range and the ids are distinct
  const size_t total = ng + (mb->rows ? 1 : 0);
  *n_out = total;
  try {
    mb->groups.reserve(ng);
  } catch (const std::bad_alloc&) {
    return fail(PSG_ERR_OOM, "host allocation");
  }
  for (size_t g = 0; g < ng; ++g)
    mb->groups.push_back(psg_minibatch::Group{h_stat[g].id, h_stat[g].start, h_stat[g].end});
  mb->groups_ok = true;
  if (total > cap) return fail(PSG_ERR_SIZE, "%zu slots, room for %zu", total, cap);
  if (total && !info) return fail(PSG_ERR_ARG, "null output");
  size_t k = 0;
  if (mb->rows) info[k++] = psg_slot_info{0, PSG_SLOT_DENSE, 0, 1, mb->rows, mb->rows};
  for (size_t g = 0; g < ng; ++g) {
    const SlotStat& t = h_stat[g];
    // parseLibsvm adds slot 1 to every example (example_parser.cc:101-102)
    const uint64_t ex = !mb->binary && t.id == 1 ? mb->rows : t.nnz_ex;
    info[k++] = psg_slot_info{(int32_t)t.id, mb->binary ? PSG_SLOT_SPARSE_BINARY : PSG_SLOT_SPARSE,
                              t.min_key, t.max_key, (uint64_t)(t.end - t.start), ex};
  }
  return PSG_OK;
}

int psg_mb_group_extract(psg_minibatch* src, int slot_id, psg_minibatch* dst) {
  using namespace psg;
  if (!src || !dst) return fail(PSG_ERR_ARG, "null argument");
  if (src == dst) return fail(PSG_ERR_ARG, "psg_mb_group_extract into its own source");
  if (src->ctx != dst->ctx) return fail(PSG_ERR_ARG, "minibatches of two contexts");
  if (slot_id < 1 || slot_id >= (int)kSlotMax) return fail(PSG_ERR_ARG, "slot id %d", slot_id);
  if (src->state != S_LOADED || !src->has_slots || !src->groups_ok)
    return fail(PSG_ERR_ARG,
                "psg_mb_group_extract needs psg_mb_groups on the source, before psg_mb_uniq");
  uint32_t start = 0, len = 0;
  for (const psg_minibatch::Group& g : src->groups)
    if (g.id == (uint32_t)slot_id) {
      start = g.start;
      len = g.end - g.start;
    }
  if ((size_t)start + len > src->nnz) return fail(PSG_ERR_DEVICE, "slot %d's segment", slot_id);
  const size_t rows = src->rows;
  const bool valued = !src->binary;
  if (int rc = mb_load_begin(dst, rows, len, valued)) return rc;
  hipStream_t s = dst->stream;  // the context's: src's too
  if (int rc = src->order(s)) return rc;
  if (len) {
    const uint32_t* seg = src->spos + start;
    LAUNCH(group_gather_kernel, blocks_of(len, 256), s, seg, len, src->at<uint64_t>(B_INDEX),
           valued ? src->at<double>(B_VALUE) : (const double*)nullptr, dst->at<uint64_t>(B_INDEX),
           dst->at<double>(B_VALUE));
    LAUNCH(group_offset_kernel, blocks_of((uint64_t)rows + 1, 256), s, src->at<uint64_t>(B_OFFSET),
           (uint32_t)rows, seg, len, dst->at<uint64_t>(B_OFFSET));
    if (int rc = launched("group extract")) return rc;
  } else {
    HIP_TRY(hipMemsetAsync(dst->b[B_OFFSET].p, 0, 8 * (rows + 1), s));
  }
  if (rows)
    HIP_TRY(hipMemcpyAsync(dst->b[B_Y].p, src->b[B_Y].p, 8 * rows, hipMemcpyDeviceToDevice, s));
  return mb_load_finish(dst, rows, len, valued);  // waits
}

int psg_even_divide(uint64_t begin, uint64_t end, size_t n, uint64_t* bounds) {
  if (n == 0 || !bounds) return fail(PSG_ERR_ARG, "psg_even_divide: n = %zu", n);
  if (end < begin) return fail(PSG_ERR_ARG, "psg_even_divide: an invalid range");
  const long double itv = (long double)(end - begin) / (long double)n;  // range.h:90-91
  for (size_t i = 0; i < n; ++i) bounds[i] = (uint64_t)(begin + itv * i);
  bounds[n] = end;  // the last partition (:93-96)
  return PSG_OK;
}

}  // extern "C"
