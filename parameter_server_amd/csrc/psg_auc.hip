// psg_auc.hip -- model evaluation resident in HBM: the reference's distributed
// AUC (src/base/auc.h:8-103: the worker's compute, the root's merge, accuracy
// and evaluate) and the exact rank AUC of Evaluation<double>::auc
// (src/base/evaluation.h:17-44).  Kernels first, the psg_auc_* entry points of
// include/psg.h after them.
//
// The histogram is the root's two maps as one table: the distinct keys in
// ascending signed order (kept with the sign bit flipped, so that unsigned
// order is signed order) and a uint64 positive and negative count per key.
//
// An add (compute fused with merge):
// (a) one key per example, k = (int64)(predict * goodness), and the batch's
//     smallest and largest key (integer atomics);
// (b) key - smallest, stably sorted with the radix passes of psg_sort.h on the
//     digits the batch's span reaches, the example's index as payload;
// (c) run heads of the sorted keys (count, scan, emit), then every run's
//     counts split by label: the lanes of a wave that share a run fold their
//     labels with ballots and one lane adds them to the run's two counters
//     (integer atomics, exact in any order);
// (d) the union with the resident table: one binary search of the table per
//     run (is the key new, and where does it go), a scan of the "new" flags,
//     and one binary search of the runs per resident entry; every entry of the
//     new table has exactly one writer.  The table ping-pongs between two sets
//     of arrays.
// A merge of host AUCData takes the same path with each entry's count as its
// weight.  No float is summed anywhere on the device.  The radix passes and
// their shape, the count / scan / emit, the binary search and the ballot fold
// are psg_sort.h's, which psg_worker.hip includes too; the handle's blocks
// are psg_blocks.h's.
//
// The exact AUC: an order-preserving key of the prediction's bits (-0.0 and
// +0.0 share one), the same sort, an exclusive scan of the "positive" flag in
// sorted order, and the sum over the negatives of that scan in uint64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/psg.h"
#include "psg_blocks.h"
#include "psg_host.h"
#include "psg_sort.h"

namespace psg {
namespace {

constexpr uint64_t kSignBit = 1ull << 63;
constexpr uint32_t kGridCap = 2048;  // workgroups of a grid-stride launch

// auc.h:75 on x86-64: a NaN product or one of magnitude >= 2^63 converts to
// INT64_MIN there (the device's own conversion saturates)
__device__ __forceinline__ uint64_t biased_key(double predict, double goodness) {
  const double p = predict * goodness;
  const long long k = fabs(p) < 9223372036854775808.0 ? (long long)p : (long long)kSignBit;
  return (uint64_t)k ^ kSignBit;
}

__device__ __forceinline__ void fold_min_max(uint64_t lo, uint64_t hi,
                                             unsigned long long* __restrict__ minmax) {
  for (int s = 32; s >= 1; s >>= 1) {
    const uint64_t a = __shfl_xor(lo, s, 64), b = __shfl_xor(hi, s, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicMin(minmax, (unsigned long long)lo);
    atomicMax(minmax + 1, (unsigned long long)hi);
  }
}

// ---- (a) ------------------------------------------------------------------
// wkey null: examples; else the keys of weighted entries
__global__ __launch_bounds__(256) void auc_keys_kernel(const double* __restrict__ predict,
                                                       const int64_t* __restrict__ wkey,
                                                       double goodness, uint32_t n,
                                                       uint64_t* __restrict__ bkey,
                                                       unsigned long long* __restrict__ minmax) {
  uint64_t lo = ~0ull, hi = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256u) {
    const uint64_t k = wkey ? (uint64_t)wkey[i] ^ kSignBit : biased_key(predict[i], goodness);
    bkey[i] = k;
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
  fold_min_max(lo, hi, minmax);
}

// ---- (b) ------------------------------------------------------------------
__global__ __launch_bounds__(256) void auc_rebase_kernel(const uint64_t* __restrict__ bkey,
                                                         uint32_t n,
                                                         const unsigned long long* __restrict__ minmax,
                                                         uint64_t* __restrict__ rkey) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) rkey[i] = bkey[i] - minmax[0];
}

// ---- (c) ------------------------------------------------------------------
// One lane per sorted item.  y: examples, positive iff y > 0 (auc.h:76).
// weight: entries, each adds its weight to the `side` counter of its run.
// cnt[0 .. n) the positive counters, cnt[n .. 2n) the negative; zeroed before.
__global__ __launch_bounds__(256) void auc_run_counts_kernel(
    const uint32_t* __restrict__ spos, const uint32_t* __restrict__ run_of,
    const double* __restrict__ y, const uint64_t* __restrict__ weight, int side, uint32_t n,
    unsigned long long* __restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool valid = i < n;
  uint32_t r = valid ? run_of[i] : 0xffffffffu;
  uint32_t at = valid ? spos[i] : 0u;
  if (at >= n) at = 0;  // never, by the sort; keeps a bad position in bounds
  if (valid && r >= n) r = n - 1;
  if (weight) {
    if (valid) atomicAdd(&cnt[(side ? (size_t)n : 0) + r], (unsigned long long)weight[at]);
    return;
  }
  const bool positive = valid && y[at] > 0;
  uint32_t cp, cn;
  if (run_label_counts(r, valid, positive, lane, &cp, &cn)) {
    if (cp) atomicAdd(&cnt[r], (unsigned long long)cp);
    if (cn) atomicAdd(&cnt[(size_t)n + r], (unsigned long long)cn);
  }
}

// ---- (d) ------------------------------------------------------------------
// words[0] = runs of the batch, words[1] = new keys among them (both uint32);
// m[0] the resident count read, m[1] the count written
// run r: its key (the batch's smallest added back), its place among the
// resident keys and whether the table lacks it
__global__ __launch_bounds__(256) void auc_run_search_kernel(
    const uint64_t* __restrict__ uniq, const uint32_t* __restrict__ words,
    const unsigned long long* __restrict__ minmax, const uint64_t* __restrict__ hkey,
    const unsigned long long* __restrict__ m_in, uint32_t n, uint64_t* __restrict__ runkey,
    uint32_t* __restrict__ lo_of, uint8_t* __restrict__ isnew) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const uint32_t nb = words[0] < n ? words[0] : n;
  if (r >= nb) {
    isnew[r] = 0;
    return;
  }
  const uint32_t m = (uint32_t)*m_in;
  const uint64_t key = uniq[r] + minmax[0];
  const uint32_t lo = lower_bound(hkey, m, key);
  runkey[r] = key;
  lo_of[r] = lo;
  isnew[r] = !(lo < m && hkey[lo] == key);
}

struct NewFlag {
  const uint8_t* isnew;
  __device__ bool operator()(uint32_t i) const { return isnew[i] != 0; }
};
struct NewEmit {  // before[i] = new keys among runs 0 .. i - 1, i = 0 .. n
  uint32_t* before;
  __device__ void operator()(uint32_t i, uint32_t ex, bool fresh, uint32_t n) const {
    before[i] = ex;
    if (i == n - 1) before[n] = ex + (fresh ? 1u : 0u);
  }
};

// the new keys of the batch go to their places; lane 0 writes the new count
__global__ __launch_bounds__(256) void auc_write_new_kernel(
    const uint64_t* __restrict__ runkey, const uint32_t* __restrict__ lo_of,
    const uint8_t* __restrict__ isnew, const uint32_t* __restrict__ before,
    const unsigned long long* __restrict__ cnt, const uint32_t* __restrict__ words, uint32_t n,
    const unsigned long long* __restrict__ m_in, unsigned long long* __restrict__ m_out,
    uint64_t* __restrict__ okey, uint64_t* __restrict__ opos, uint64_t* __restrict__ oneg,
    uint32_t cap) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r == 0) *m_out = *m_in + before[n];
  const uint32_t nb = words[0] < n ? words[0] : n;
  if (r >= nb || !isnew[r]) return;
  const uint64_t out = (uint64_t)lo_of[r] + before[r];
  if (out < cap) {  // always: the host keeps resident + batch within cap
    okey[out] = runkey[r];
    opos[out] = cnt[r];
    oneg[out] = cnt[(size_t)n + r];
  }
}

// resident entry j moves up by the new keys below it and takes its run's counts
__global__ __launch_bounds__(256) void auc_write_resident_kernel(
    const uint64_t* __restrict__ hkey, const uint64_t* __restrict__ hpos,
    const uint64_t* __restrict__ hneg, const unsigned long long* __restrict__ m_in,
    const uint64_t* __restrict__ runkey, const uint32_t* __restrict__ before,
    const unsigned long long* __restrict__ cnt, const uint32_t* __restrict__ words, uint32_t n,
    uint64_t* __restrict__ okey, uint64_t* __restrict__ opos, uint64_t* __restrict__ oneg,
    uint32_t cap) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t m = (uint32_t)*m_in;
  if (j >= m || j >= cap) return;
  const uint32_t nb = words[0] < n ? words[0] : n;
  const uint64_t key = hkey[j];
  const uint32_t lb = lower_bound(runkey, nb, key);
  const bool hit = lb < nb && runkey[lb] == key;
  const uint64_t out = j + before[lb];
  if (out < cap) {
    okey[out] = key;
    opos[out] = hpos[j] + (hit ? cnt[lb] : 0ull);
    oneg[out] = hneg[j] + (hit ? cnt[(size_t)n + lb] : 0ull);
  }
}

// ---- the exact AUC ----------------------------------------------------------
// ascending key = ascending prediction under a.predict < b.predict; the two
// zeros compare equal there and share a key.  nan += the NaN predictions.
__global__ __launch_bounds__(256) void exact_keys_kernel(const double* __restrict__ predict,
                                                         uint32_t n, uint64_t* __restrict__ key,
                                                         unsigned long long* __restrict__ nan) {
  uint32_t bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256u) {
    const double p = predict[i];
    if (p != p) ++bad;
    const uint64_t b = p == 0 ? 0ull : (uint64_t)__double_as_longlong(p);
    key[i] = (b & kSignBit) ? ~b : b | kSignBit;
  }
  if (bad) atomicAdd(nan, (unsigned long long)bad);
}

struct PositiveFlag {  // sorted example i is a positive (evaluation.h:36)
  const double* y;
  const uint32_t* spos;
  uint32_t n;
  __device__ bool operator()(uint32_t i) const {
    const uint32_t at = spos[i];
    return at < n && y[at] > 0;
  }
};
struct AreaEmit {  // ex: positives sorted before example i; a negative adds it
  uint32_t* term;
  __device__ void operator()(uint32_t i, uint32_t ex, bool positive, uint32_t) const {
    term[i] = positive ? 0u : ex;
  }
};

__global__ __launch_bounds__(256) void sum_u32_kernel(const uint32_t* __restrict__ v, uint32_t n,
                                                      unsigned long long* __restrict__ total) {
  uint64_t a = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256u)
    a += v[i];
  for (int s = 32; s >= 1; s >>= 1) a += __shfl_xor(a, s, 64);
  if ((threadIdx.x & 63u) == 0 && a) atomicAdd(total, (unsigned long long)a);
}

// every bit up to the highest one of `span`: the digits two keys within that
// span of each other can differ in (after the smallest is subtracted)
inline uint64_t bits_up_to(uint64_t span) {
  uint64_t b = 0;
  while (b < span) b = (b << 1) | 1u;
  return b;
}

}  // namespace
}  // namespace psg

// ------------------------------------------------------------------- host --
using psg::fail;

namespace {

enum AucBuf {
  A_Y, A_PREDICT, A_WKEY, A_WCNT, A_BKEY, A_KEY_A, A_KEY_B, A_POS_A, A_POS_B, A_COUNTS,
  A_TILE_SUM, A_UNIQ, A_RUN_START, A_RUN_OF, A_CNT, A_RUNKEY, A_LO, A_ISNEW, A_BEFORE, A_COUNT
};

// device words: [0] smallest key of the batch, [1] largest, [2] [3] the
// resident count of either side of the ping-pong, [4] as two u32: runs of the
// batch, new keys among them; then the 256 digit totals
constexpr size_t kAucSmallBytes = 5 * 8 + 256 * 4;

}  // namespace

struct psg_auc : psg::DeviceBlocks<A_COUNT> {
  int64_t goodness = 0;
  // the table: two sets of key / pos / neg arrays of `cap` entries each
  uint64_t* tab[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  size_t cap = 0;
  int cur = 0;       // the set that holds the table
  size_t bound = 0;  // the resident count is at most this

  unsigned long long* d_m(int side) const { return d_small + 2 + side; }
  uint32_t* d_words() const { return (uint32_t*)(d_small + 4); }
  uint32_t* d_dtotal() const { return (uint32_t*)(d_small + 5); }
};

namespace {

using namespace psg;

constexpr size_t kMaxItems = 0xffffffffull;  // positions and ranks are uint32

// The true resident count, after a wait.
int read_count(psg_auc* h, size_t* m) {
  if (int rc = h->settle()) return rc;
  HIP_TRY(hipMemcpy(h->h_small + 2, h->d_m(h->cur), 8, hipMemcpyDeviceToHost));
  *m = (size_t)h->h_small[2];
  if (*m > h->cap) return fail(PSG_ERR_DEVICE, "%zu histogram entries in room for %zu", *m, h->cap);
  h->bound = *m;
  return PSG_OK;
}

// Room for `add` more keys.  Follows psg_ftrl_reserve: the host's bound grows
// by every add's item count, and the device's count is read only when the
// bound passes the capacity.
int make_room(psg_auc* h, size_t add) {
  if (h->bound + add <= h->cap) return PSG_OK;
  size_t m = 0;
  if (h->cap) {
    if (int rc = read_count(h, &m)) return rc;
    if (m + add <= h->cap) return PSG_OK;
  }
  if (m + add >= kMaxItems) return fail(PSG_ERR_SIZE, "%zu histogram keys >= 2^32 - 1", m + add);
  const size_t cap = std::min(kMaxItems, std::max<size_t>({2 * h->cap, m + add, (size_t)1 << 16}));
  uint64_t* fresh[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  for (auto& set : fresh)
    for (auto& p : set)
      if (hipMalloc((void**)&p, 8 * cap) != hipSuccess) {
        (void)hipGetLastError();
        for (auto& set2 : fresh)
          for (auto& q : set2)
            if (q) (void)hipFree(q);
        return fail(PSG_ERR_OOM, "histogram of %zu entries", cap);
      }
  for (int a = 0; a < 3; ++a)
    if (m) HIP_TRY(hipMemcpy(fresh[h->cur][a], h->tab[h->cur][a], 8 * m, hipMemcpyDeviceToDevice));
  for (int sd = 0; sd < 2; ++sd)
    for (int a = 0; a < 3; ++a) {
      if (h->tab[sd][a]) (void)hipFree(h->tab[sd][a]);
      h->tab[sd][a] = fresh[sd][a];
    }
  h->cap = cap;
  return PSG_OK;
}

// n items into the table: examples (y, predict) or weighted entries (wkey,
// weight, all of them positives' (side 0) or negatives' (side 1)); device arrays
int add_items(psg_auc* h, size_t n_z, const double* y, const double* predict,
              const int64_t* wkey, const uint64_t* weight, int side, hipStream_t s) {
  if (n_z >= kMaxItems) return fail(PSG_ERR_SIZE, "%zu items >= 2^32 - 1", n_z);
  if (n_z == 0) return PSG_OK;
  if (int rc = make_room(h, n_z)) return rc;
  const uint32_t n = (uint32_t)n_z, ntiles = blocks_of(n, kSortTile), nt = blocks_of(n, kFlagTile);
  if (int rc = h->need_all({
      {A_BKEY, 8 * n_z}, {A_KEY_A, 8 * n_z}, {A_KEY_B, 8 * n_z}, {A_POS_A, 4 * n_z},
      {A_POS_B, 4 * n_z}, {A_COUNTS, 4 * 256 * (size_t)ntiles}, {A_TILE_SUM, 4 * (size_t)nt + 4},
      {A_UNIQ, 8 * n_z}, {A_RUN_START, 4 * (n_z + 1)}, {A_RUN_OF, 4 * n_z}, {A_CNT, 16 * n_z},
      {A_RUNKEY, 8 * n_z}, {A_LO, 4 * n_z}, {A_ISNEW, n_z}, {A_BEFORE, 4 * (n_z + 1)}}))
    return rc;
  if (int rc = h->order(s)) return rc;
  // (a)
  h->h_small[0] = ~0ull;
  h->h_small[1] = 0;
  HIP_TRY(hipMemcpyAsync(h->d_small, h->h_small, 16, hipMemcpyHostToDevice, s));
  uint64_t* bkey = h->at<uint64_t>(A_BKEY);
  LAUNCH(auc_keys_kernel, std::min(blocks_of(n, 256), kGridCap), s, predict, wkey,
         (double)h->goodness, n, bkey, h->d_small);
  if (int rc = launched("auc keys")) return rc;
#ifdef PSG_AUC_EIGHT_PASSES  // A/B build: no host wait, every digit sorted on
  const uint64_t differ = ~0ull;
#else
  // The batch's span decides which digits are sorted on: the host reads these
  // two words, as psg_mb_load reads its OR / AND.
  HIP_TRY(hipMemcpyAsync(h->h_small, h->d_small, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h->h_small[0] > h->h_small[1]) return fail(PSG_ERR_DEVICE, "auc keys: no key range");
  const uint64_t differ = bits_up_to(h->h_small[1] - h->h_small[0]);
#endif
  // (b)
  uint64_t* rkey = h->at<uint64_t>(A_KEY_B);
  LAUNCH(auc_rebase_kernel, blocks_of(n, 256), s, bkey, n, h->d_small, rkey);
  const SortBuffers sb{h->at<uint64_t>(A_KEY_A), h->at<uint64_t>(A_KEY_B), h->at<uint32_t>(A_POS_A),
                       h->at<uint32_t>(A_POS_B), h->at<uint32_t>(A_COUNTS), h->d_dtotal()};
  const uint64_t* skey = nullptr;
  const uint32_t* spos = nullptr;
  if (int rc = enqueue_radix_sort(rkey, n, differ, sb, &skey, &spos, s)) return rc;
  // (c)
  uint32_t* ts = h->at<uint32_t>(A_TILE_SUM);
  unsigned long long* cnt = h->at<unsigned long long>(A_CNT);
  const HeadFlag hf{skey};
  const HeadEmit he{skey, h->at<uint64_t>(A_UNIQ), h->at<uint32_t>(A_RUN_START),
                    h->at<uint32_t>(A_RUN_OF)};
  enqueue_flag_scan(hf, he, n, ts, h->d_words(), s);
  HIP_TRY(hipMemsetAsync(cnt, 0, 16 * n_z, s));
  LAUNCH(auc_run_counts_kernel, blocks_of(n, 256), s, spos, h->at<uint32_t>(A_RUN_OF), y, weight,
         side, n, cnt);
  // (d)
  const int cur = h->cur, nxt = cur ^ 1;
  const uint32_t cap = (uint32_t)h->cap;
  uint64_t* runkey = h->at<uint64_t>(A_RUNKEY);
  uint32_t* lo_of = h->at<uint32_t>(A_LO);
  uint8_t* isnew = h->at<uint8_t>(A_ISNEW);
  uint32_t* before = h->at<uint32_t>(A_BEFORE);
  LAUNCH(auc_run_search_kernel, blocks_of(n, 256), s, h->at<uint64_t>(A_UNIQ), h->d_words(),
         h->d_small, h->tab[cur][0], h->d_m(cur), n, runkey, lo_of, isnew);
  const NewFlag nf{isnew};
  const NewEmit ne{before};
  enqueue_flag_scan(nf, ne, n, ts, h->d_words() + 1, s);
  LAUNCH(auc_write_new_kernel, blocks_of(n, 256), s, runkey, lo_of, isnew, before, cnt,
         h->d_words(), n, h->d_m(cur), h->d_m(nxt), h->tab[nxt][0], h->tab[nxt][1],
         h->tab[nxt][2], cap);
  if (h->bound)
    LAUNCH(auc_write_resident_kernel, blocks_of(h->bound, 256), s, h->tab[cur][0], h->tab[cur][1],
           h->tab[cur][2], h->d_m(cur), runkey, before, cnt, h->d_words(), n, h->tab[nxt][0],
           h->tab[nxt][1], h->tab[nxt][2], cap);
  if (int rc = launched("auc add")) return rc;
  h->cur = nxt;
  h->bound += n_z;
  return h->mark(s);
}

// the table as the AUCData of auc.h:85-97, after a wait
int export_lists(psg_auc* h, std::vector<int64_t>* tk, std::vector<uint64_t>* tc,
                 std::vector<int64_t>* fk, std::vector<uint64_t>* fc) {
  HIP_TRY(hipSetDevice(h->device));
  size_t m = 0;
  if (h->cap)
    if (int rc = read_count(h, &m)) return rc;
  try {
    std::vector<uint64_t> key(m), pos(m), neg(m);
    if (m) {
      HIP_TRY(hipMemcpy(key.data(), h->tab[h->cur][0], 8 * m, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(pos.data(), h->tab[h->cur][1], 8 * m, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(neg.data(), h->tab[h->cur][2], 8 * m, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < m; ++i) {
      const int64_t k = (int64_t)(key[i] ^ kSignBit);
      if (pos[i]) {
        tk->push_back(k);
        tc->push_back(pos[i]);
      }
      if (neg[i]) {
        fk->push_back(k);
        fc->push_back(neg[i]);
      }
    }
  } catch (const std::bad_alloc&) {
    return fail(PSG_ERR_OOM, "host allocation");
  }
  return PSG_OK;
}

}  // namespace

extern "C" {

int psg_auc_create(psg_ctx* ctx, int64_t goodness, psg_auc** out) {
  if (!ctx || !out) return fail(PSG_ERR_ARG, "null argument");
  *out = nullptr;
  int device, dtype;
  hipStream_t stream;
  psg::ctx_info(ctx, &device, &dtype, &stream);
  HIP_TRY(hipSetDevice(device));
  psg_auc* h = new (std::nothrow) psg_auc();
  if (!h) return fail(PSG_ERR_OOM, "host allocation");
  h->goodness = goodness;
  if (!h->open(ctx, kAucSmallBytes) ||
      hipMemset(h->d_small, 0, kAucSmallBytes) != hipSuccess) {
    (void)hipGetLastError();
    psg_auc_destroy(h);
    return fail(PSG_ERR_OOM, "auc control blocks");
  }
  *out = h;
  return PSG_OK;
}

void psg_auc_destroy(psg_auc* h) {
  if (!h) return;
  h->close();
  for (auto& set : h->tab)
    for (auto& p : set)
      if (p) (void)hipFree(p);
  delete h;
}

int psg_auc_clear(psg_auc* h) {
  if (!h) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (int rc = h->order(s)) return rc;
  HIP_TRY(hipMemsetAsync(h->d_m(0), 0, 16, s));
  h->bound = 0;
  return h->mark(s);
}

int psg_auc_set_goodness(psg_auc* h, int64_t goodness) {
  if (!h) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  size_t m = 0;
  if (h->bound && h->cap)
    if (int rc = read_count(h, &m)) return rc;
  if (m) return fail(PSG_ERR_ARG, "psg_auc_set_goodness on a histogram of %zu keys", m);
  h->goodness = goodness;
  return PSG_OK;
}

int psg_auc_add_dev(psg_auc* h, const double* y_dev, const double* predict_dev, size_t n,
                    void* stream) {
  if (!h || (n && (!y_dev || !predict_dev))) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  return add_items(h, n, y_dev, predict_dev, nullptr, nullptr, 0, h->pick(stream));
}

int psg_auc_add(psg_auc* h, const double* y, const double* predict, size_t n) {
  if (!h || (n && (!y || !predict))) return fail(PSG_ERR_ARG, "null argument");
  if (n >= kMaxItems) return fail(PSG_ERR_SIZE, "%zu examples >= 2^32 - 1", n);
  if (n == 0) return PSG_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (int rc = h->settle()) return rc;  // the staging blocks may be in use
  if (int rc = h->need(A_Y, 8 * n)) return rc;
  if (int rc = h->need(A_PREDICT, 8 * n)) return rc;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(h->b[A_Y].p, y, 8 * n, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->b[A_PREDICT].p, predict, 8 * n, hipMemcpyHostToDevice, s));
  return add_items(h, n, h->at<double>(A_Y), h->at<double>(A_PREDICT), nullptr, nullptr, 0, s);
}

int psg_auc_merge(psg_auc* h, const int64_t* tp_key, const uint64_t* tp_count, size_t ntp,
                  const int64_t* fp_key, const uint64_t* fp_count, size_t nfp) {
  if (!h || (ntp && (!tp_key || !tp_count)) || (nfp && (!fp_key || !fp_count)))
    return fail(PSG_ERR_ARG, "null argument");
  if (ntp >= kMaxItems || nfp >= kMaxItems)
    return fail(PSG_ERR_SIZE, "%zu + %zu entries >= 2^32 - 1", ntp, nfp);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  for (int side = 0; side < 2; ++side) {
    const int64_t* key = side ? fp_key : tp_key;
    const uint64_t* count = side ? fp_count : tp_count;
    const size_t n = side ? nfp : ntp;
    std::vector<int64_t> k;
    std::vector<uint64_t> c;
    try {
      for (size_t i = 0; i < n; ++i)
        if (count[i]) {  // an entry that counts nothing makes no key
          k.push_back(key[i]);
          c.push_back(count[i]);
        }
    } catch (const std::bad_alloc&) {
      return fail(PSG_ERR_OOM, "host allocation");
    }
    if (k.empty()) continue;
    if (int rc = h->settle()) return rc;  // the staging blocks may be in use
    if (int rc = h->need(A_WKEY, 8 * k.size())) return rc;
    if (int rc = h->need(A_WCNT, 8 * k.size())) return rc;
    HIP_TRY(hipMemcpy(h->b[A_WKEY].p, k.data(), 8 * k.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->b[A_WCNT].p, c.data(), 8 * c.size(), hipMemcpyHostToDevice));
    if (int rc = add_items(h, k.size(), nullptr, nullptr, h->at<int64_t>(A_WKEY),
                           h->at<uint64_t>(A_WCNT), side, s))
      return rc;
  }
  return PSG_OK;
}

int psg_auc_data(psg_auc* h, int64_t* tp_key, uint64_t* tp_count, size_t tp_cap, size_t* ntp,
                 int64_t* fp_key, uint64_t* fp_count, size_t fp_cap, size_t* nfp) {
  if (!h || !ntp || !nfp) return fail(PSG_ERR_ARG, "null argument");
  *ntp = *nfp = 0;
  std::vector<int64_t> tk, fk;
  std::vector<uint64_t> tc, fc;
  if (int rc = export_lists(h, &tk, &tc, &fk, &fc)) return rc;
  *ntp = tk.size();
  *nfp = fk.size();
  if (tk.size() > tp_cap || fk.size() > fp_cap)
    return fail(PSG_ERR_SIZE, "psg_auc_data: %zu + %zu entries, room for %zu + %zu", tk.size(),
                fk.size(), tp_cap, fp_cap);
  if ((tk.size() && (!tp_key || !tp_count)) || (fk.size() && (!fp_key || !fp_count)))
    return fail(PSG_ERR_ARG, "null output");
  if (!tk.empty()) {
    memcpy(tp_key, tk.data(), 8 * tk.size());
    memcpy(tp_count, tc.data(), 8 * tc.size());
  }
  if (!fk.empty()) {
    memcpy(fp_key, fk.data(), 8 * fk.size());
    memcpy(fp_count, fc.data(), 8 * fc.size());
  }
  return PSG_OK;
}

int psg_auc_accuracy_data(int64_t goodness, const int64_t* tp_key, const uint64_t* tp_count,
                          size_t ntp, const int64_t* fp_key, const uint64_t* fp_count, size_t nfp,
                          double threshold, double* out) {
  if (!out || (ntp && (!tp_key || !tp_count)) || (nfp && (!fp_key || !fp_count)))
    return fail(PSG_ERR_ARG, "null argument");
  double total = 0, correct = 0;
  const double x = threshold * goodness;
  for (size_t i = 0; i < ntp; ++i) {
    if (tp_key[i] >= x) correct += tp_count[i];
    total += tp_count[i];
  }
  for (size_t i = 0; i < nfp; ++i) {
    if (fp_key[i] < x) correct += fp_count[i];
    total += fp_count[i];
  }
  *out = correct / total;
  return PSG_OK;
}

int psg_auc_evaluate_data(const int64_t* tp_key, const uint64_t* tp_count, size_t ntp,
                          const int64_t* fp_key, const uint64_t* fp_count, size_t nfp, int mode,
                          double* out) {
  if (!out || (ntp && (!tp_key || !tp_count)) || (nfp && (!fp_key || !fp_count)))
    return fail(PSG_ERR_ARG, "null argument");
  if (mode != PSG_AUC_BY_KEY && mode != PSG_AUC_AS_WRITTEN)
    return fail(PSG_ERR_ARG, "psg_auc_evaluate: mode %d", mode);
  if (ntp == 0 || nfp == 0) {
    *out = 0.5;
    return PSG_OK;
  }
  double tp_sum = 0, fp_sum = 0, auc = 0;
  size_t t = 0;
  for (size_t f = 0; f < nfp; ++f) {
    const uint64_t fp_v = fp_count[f];
    for (; t < ntp && (mode == PSG_AUC_BY_KEY ? tp_key[t] <= fp_key[f] : tp_count[t] <= fp_v); ++t)
      tp_sum += tp_count[t];
    fp_sum += fp_v;
    auc += tp_sum * fp_v;
  }
  for (; t < ntp; ++t) tp_sum += tp_count[t];
  auc = auc / tp_sum / fp_sum;
  *out = auc < .5 ? 1 - auc : auc;
  return PSG_OK;
}

int psg_auc_accuracy(psg_auc* h, double threshold, double* v) {
  if (!h || !v) return fail(PSG_ERR_ARG, "null argument");
  std::vector<int64_t> tk, fk;
  std::vector<uint64_t> tc, fc;
  if (int rc = export_lists(h, &tk, &tc, &fk, &fc)) return rc;
  return psg_auc_accuracy_data(h->goodness, tk.data(), tc.data(), tk.size(), fk.data(), fc.data(),
                               fk.size(), threshold, v);
}

int psg_auc_evaluate(psg_auc* h, int mode, double* v) {
  if (!h || !v) return fail(PSG_ERR_ARG, "null argument");
  std::vector<int64_t> tk, fk;
  std::vector<uint64_t> tc, fc;
  if (int rc = export_lists(h, &tk, &tc, &fk, &fc)) return rc;
  return psg_auc_evaluate_data(tk.data(), tc.data(), tk.size(), fk.data(), fc.data(), fk.size(),
                               mode, v);
}

int psg_auc_exact_dev(psg_ctx* ctx, const double* y_dev, const double* predict_dev, size_t n_z,
                      double* auc, void* stream) {
  if (!ctx || !auc || (n_z && (!y_dev || !predict_dev))) return fail(PSG_ERR_ARG, "null argument");
  if (n_z >= kMaxItems) return fail(PSG_ERR_SIZE, "%zu examples >= 2^32 - 1", n_z);
  const double zero = 0.0;
  if (n_z == 0) {
    *auc = zero / zero;  // area /= 0 * 0, evaluation.h:42
    return PSG_OK;
  }
  int device, dtype;
  hipStream_t cs;
  psg::ctx_info(ctx, &device, &dtype, &cs);
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = stream ? (hipStream_t)stream : cs;
  const uint32_t n = (uint32_t)n_z, ntiles = blocks_of(n, kSortTile), nt = blocks_of(n, kFlagTile);
  // one block: the small words, then every array (each a multiple of 8 bytes)
  // words: [0] OR of the keys, [1] AND, [2] NaN predictions, [3] the area,
  // [4] as u32: the positives; then the 256 digit totals
  const size_t small = 5 * 8 + 256 * 4;
  const size_t r8 = (4 * n_z + 7) / 8 * 8;
  const size_t sizes[] = {small, 8 * n_z, 8 * n_z, 8 * n_z, r8, r8, 4 * 256 * (size_t)ntiles,
                          (4 * (size_t)nt + 4 + 7) / 8 * 8, r8};
  size_t off[10] = {0};
  for (int i = 0; i < 9; ++i) off[i + 1] = off[i] + sizes[i];
  char* base = nullptr;
  HIP_TRY(hipMalloc((void**)&base, off[9]));
  unsigned long long h_small[5] = {0, ~0ull, 0, 0, 0};
  int rc = [&]() -> int {
    unsigned long long* d_small = (unsigned long long*)base;
    uint64_t* key = (uint64_t*)(base + off[1]);
    const SortBuffers sb{(uint64_t*)(base + off[2]), (uint64_t*)(base + off[3]),
                         (uint32_t*)(base + off[4]), (uint32_t*)(base + off[5]),
                         (uint32_t*)(base + off[6]), (uint32_t*)(d_small + 5)};
    uint32_t* ts = (uint32_t*)(base + off[7]);
    uint32_t* term = (uint32_t*)(base + off[8]);
    HIP_TRY(hipMemcpyAsync(d_small, h_small, sizeof h_small, hipMemcpyHostToDevice, s));
    const uint32_t grid = std::min(blocks_of(n, 256), kGridCap);
    LAUNCH(exact_keys_kernel, grid, s, predict_dev, n, key, d_small + 2);
    LAUNCH(key_bits_kernel, grid, s, key, n, d_small);
    if (int e = launched("exact auc keys")) return e;
    HIP_TRY(hipMemcpyAsync(h_small, d_small, 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h_small[2])  // the comparator is no strict weak order then
      return fail(PSG_ERR_ARG, "psg_auc_exact: %llu NaN predictions", h_small[2]);
    const uint64_t* skey = nullptr;
    const uint32_t* spos = nullptr;
    if (int e = enqueue_radix_sort(key, n, h_small[0] ^ h_small[1], sb, &skey, &spos, s)) return e;
    const PositiveFlag pf{y_dev, spos, n};
    const AreaEmit ae{term};
    enqueue_flag_scan(pf, ae, n, ts, (uint32_t*)(d_small + 4), s);
    LAUNCH(sum_u32_kernel, grid, s, term, n, d_small + 3);
    if (int e = launched("exact auc")) return e;
    HIP_TRY(hipMemcpyAsync(h_small + 3, d_small + 3, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return PSG_OK;
  }();
  if (rc != PSG_OK) (void)hipStreamSynchronize(s);
  (void)hipFree(base);
  if (rc != PSG_OK) return rc;
  const uint64_t pos = h_small[4] & 0xffffffffull;
  if (pos > n_z) return fail(PSG_ERR_DEVICE, "%llu positives of %zu examples",
                             (unsigned long long)pos, n_z);
  double area = (double)h_small[3];
  area /= (double)pos * (double)(n_z - pos);  // evaluation.h:42
  *auc = area < 0.5 ? 1 - area : area;
  return PSG_OK;
}

int psg_auc_exact(psg_ctx* ctx, const double* y, const double* predict, size_t n, double* auc) {
  if (!ctx || !auc || (n && (!y || !predict))) return fail(PSG_ERR_ARG, "null argument");
  if (n >= kMaxItems) return fail(PSG_ERR_SIZE, "%zu examples >= 2^32 - 1", n);
  if (n == 0) return psg_auc_exact_dev(ctx, nullptr, nullptr, 0, auc, nullptr);
  int device, dtype;
  hipStream_t cs;
  psg::ctx_info(ctx, &device, &dtype, &cs);
  HIP_TRY(hipSetDevice(device));
  double* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 16 * n));
  int rc = PSG_OK;
  if (hipMemcpy(d, y, 8 * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d + n, predict, 8 * n, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    rc = fail(PSG_ERR_DEVICE, "psg_auc_exact: copy to the device");
  }
  if (rc == PSG_OK) rc = psg_auc_exact_dev(ctx, d, d + n, n, auc, nullptr);
  (void)hipFree(d);
  return rc;
}

}  // extern "C"
