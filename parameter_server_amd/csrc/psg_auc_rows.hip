// psg_auc_rows.hip -- the histogram AUC of psg_auc.hip for row-valued
// predictions: m histograms (one per model of a sweep) kept
// as ONE table and updated by one sort, one run pass and one union per
// minibatch.  Kernels first, the psg_auc_rows_* entry
// points of include/psg.h after them.
//
// The table: the m histograms concatenated in (model, key) order -- keys with
// the sign bit flipped, a uint64 positive and negative count per key -- and
// seg[m + 1], model j's entries being [seg[j], seg[j + 1]).  Both ping-pong.
//
// A pass folds N items into the table.  Item t has a model, a source word and
// a label row; the three shapes of a pass are
//   all models   t = i * m + j: model j, word t of predict, row i  (an add);
//   one model    model j, word t * m + j of predict, row t  (a wide add, below);
//   entries      model j, word t of the merged keys, its own weight  (a merge).
// (a) the scalar path's key per item, and ONE smallest and largest key for
//     all models (a wave folds its lanes before the two atomics);
// (b) with b the width of largest - smallest and c = ceil(log2 m): the item's
//     composite key (field << b) | (key - smallest), field its model minus the
//     pass's first, sorted once by psg_sort.h's radix passes on the digits
//     that b + c bits reach, t as payload;
// (c) run heads over the composite keys, then every run's counts by the
//     wave's ballot fold (a weighted item adds its weight itself);
// (d) the union: a run decodes (model, key) and searches its model's segment;
//     the "new" flags are scanned; a new run goes to its place plus the new
//     runs before it; a resident entry finds its model from seg (in LDS),
//     forms its own composite key and searches the runs once; each boundary
//     of the new seg searches the runs for its model's first.  Every word of
//     the new table and of the new seg has one writer; no atomics.
// b + c > 64 (a key of INT64_MIN beside ordinary ones, or a large goodness):
// the add runs model by model through the same kernels as m one-model passes,
// where c = 0 and every span fits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/psg.h"
#include "psg_auc_dev.h"
#include "psg_blocks.h"
#include "psg_host.h"
#include "psg_sort.h"

namespace psg {
namespace {

constexpr uint32_t kSegWords = PSG_FTRL_MAX_MODELS + 1;

// The shape of a pass.  models > 1: item t is model first + t % models, its
// source word is t and its label row t / models.  models == 1: every item is
// model `first`, its source word t * stride + off and its label row t.
struct Pass {
  uint32_t models, first, stride, off;
  uint32_t b;  // the width of largest - smallest key (set once the span is read)
};

__device__ __forceinline__ uint64_t low_bits(uint32_t b) { return b >= 64 ? ~0ull : (1ull << b) - 1; }
// models > 1 keeps b < 64; with one model the field is 0
__device__ __forceinline__ uint64_t compose(uint32_t field, uint64_t rel, uint32_t b) {
  return b >= 64 ? rel : ((uint64_t)field << b) | rel;
}

// runs ordered before (field f, key): the composite keys `uniq` ascend by
// (field, key - smallest).  *at = the key's composite where it lies within the
// batch's span (else no run can equal it: *inside false).
__device__ __forceinline__ uint32_t runs_before(const uint64_t* __restrict__ uniq, uint32_t nb,
                                                const Pass& P, int64_t f, uint64_t key,
                                                uint64_t lo_key, uint64_t hi_key, uint64_t* at,
                                                bool* inside) {
  *inside = false;
  if (f < 0) return 0;
  if (f >= (int64_t)P.models) return nb;
  if (key > hi_key)  // past every run of its model
    return f + 1 >= (int64_t)P.models ? nb : lower_bound(uniq, nb, compose((uint32_t)f + 1, 0, P.b));
  *inside = key >= lo_key;
  *at = compose((uint32_t)f, *inside ? key - lo_key : 0, P.b);
  return lower_bound(uniq, nb, *at);
}

// ---- (a) ------------------------------------------------------------------
// wkey null: predictions; else the keys of weighted entries
__global__ __launch_bounds__(256) void aucr_keys_kernel(const double* __restrict__ predict,
                                                        const int64_t* __restrict__ wkey,
                                                        double goodness, uint32_t n, Pass P,
                                                        uint64_t* __restrict__ bkey,
                                                        unsigned long long* __restrict__ minmax) {
  uint64_t lo = ~0ull, hi = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < n;
       t += (uint64_t)gridDim.x * 256u) {
    const uint64_t k = wkey ? (uint64_t)wkey[t] ^ kSignBit
                            : biased_key(predict[t * P.stride + P.off], goodness);
    bkey[t] = k;
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
  fold_min_max(lo, hi, minmax);
}

// ---- (b) ------------------------------------------------------------------
__global__ __launch_bounds__(256) void aucr_compose_kernel(
    const uint64_t* __restrict__ bkey, uint32_t n, Pass P,
    const unsigned long long* __restrict__ minmax, uint64_t* __restrict__ ckey) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint32_t field = P.models > 1 ? (uint32_t)t % P.models : 0u;
  ckey[t] = compose(field, bkey[t] - minmax[0], P.b);
}

// ---- (c) ------------------------------------------------------------------
// One lane per sorted item.  y: the label of the item's row, positive iff
// y > 0.  weight: entries, each adds its weight to the `side` counter of its
// run.  cnt[0 .. n) the positive counters, cnt[n .. 2n) the negative; zeroed.
__global__ __launch_bounds__(256) void aucr_run_counts_kernel(
    const uint32_t* __restrict__ spos, const uint32_t* __restrict__ run_of,
    const double* __restrict__ y, const uint64_t* __restrict__ weight, int side, uint32_t n,
    uint32_t models, unsigned long long* __restrict__ cnt) {
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
  const bool positive = valid && y[models > 1 ? at / models : at] > 0;
  uint32_t cp, cn;
  if (run_label_counts(r, valid, positive, lane, &cp, &cn)) {
    if (cp) atomicAdd(&cnt[r], (unsigned long long)cp);
    if (cn) atomicAdd(&cnt[(size_t)n + r], (unsigned long long)cn);
  }
}

// ---- (d) ------------------------------------------------------------------
// the workgroup's copy of seg[0 .. m]; every lane of the workgroup comes here
__device__ __forceinline__ void load_seg(const uint32_t* __restrict__ seg, uint32_t m,
                                         uint32_t* lds) {
  if (threadIdx.x <= m) lds[threadIdx.x] = seg[threadIdx.x];
  __syncthreads();
}

// words[0] = runs of the pass, words[1] = new keys among them.  Run r: its
// key (the smallest added back), its place in the table and whether its
// model's segment lacks it
__global__ __launch_bounds__(256) void aucr_run_search_kernel(
    const uint64_t* __restrict__ uniq, const uint32_t* __restrict__ words,
    const unsigned long long* __restrict__ minmax, const uint64_t* __restrict__ hkey,
    const uint32_t* __restrict__ seg_in, uint32_t m, Pass P, uint32_t n,
    uint64_t* __restrict__ runkey, uint32_t* __restrict__ lo_of, uint8_t* __restrict__ isnew) {
  __shared__ uint32_t seg[kSegWords];
  load_seg(seg_in, m, seg);
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const uint32_t nb = words[0] < n ? words[0] : n;
  if (r >= nb) {
    isnew[r] = 0;
    return;
  }
  const uint64_t c = uniq[r];
  uint32_t j = P.first + (P.b >= 64 ? 0u : (uint32_t)(c >> P.b));
  if (j >= m) j = m - 1;  // never, by the compose
  const uint64_t key = (c & low_bits(P.b)) + minmax[0];
  const uint32_t s0 = seg[j], s1 = seg[j + 1] > s0 ? seg[j + 1] : s0;
  const uint32_t lo = s0 + lower_bound(hkey + s0, s1 - s0, key);
  runkey[r] = key;
  lo_of[r] = lo;
  isnew[r] = !(lo < s1 && hkey[lo] == key);
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

// the new runs go to their places; lanes 0 .. m of the first workgroup write
// the new seg: boundary j moves up by the new runs of the models before j
__global__ __launch_bounds__(256) void aucr_write_new_kernel(
    const uint64_t* __restrict__ uniq, const uint64_t* __restrict__ runkey,
    const uint32_t* __restrict__ lo_of, const uint8_t* __restrict__ isnew,
    const uint32_t* __restrict__ before, const unsigned long long* __restrict__ cnt,
    const uint32_t* __restrict__ words, uint32_t n, const uint32_t* __restrict__ seg_in,
    uint32_t* __restrict__ seg_out, uint32_t m, Pass P, uint64_t* __restrict__ okey,
    uint64_t* __restrict__ opos, uint64_t* __restrict__ oneg, uint32_t cap) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t nb = words[0] < n ? words[0] : n;
  if (r <= m) {
    const int64_t f = (int64_t)r - (int64_t)P.first;
    const uint32_t lb = f <= 0 ? 0u
                        : f >= (int64_t)P.models ? nb
                                                 : lower_bound(uniq, nb, compose((uint32_t)f, 0, P.b));
    seg_out[r] = seg_in[r] + before[lb];
  }
  if (r >= nb || !isnew[r]) return;
  const uint64_t out = (uint64_t)lo_of[r] + before[r];
  if (out < cap) {  // always: the host keeps resident + batch within cap
    okey[out] = runkey[r];
    opos[out] = cnt[r];
    oneg[out] = cnt[(size_t)n + r];
  }
}

// resident entry e moves up by the new runs ordered before it and takes its
// run's counts
__global__ __launch_bounds__(256) void aucr_write_resident_kernel(
    const uint64_t* __restrict__ hkey, const uint64_t* __restrict__ hpos,
    const uint64_t* __restrict__ hneg, const uint32_t* __restrict__ seg_in, uint32_t m, Pass P,
    const uint64_t* __restrict__ uniq, const unsigned long long* __restrict__ minmax,
    const uint32_t* __restrict__ before, const unsigned long long* __restrict__ cnt,
    const uint32_t* __restrict__ words, uint32_t n, uint64_t* __restrict__ okey,
    uint64_t* __restrict__ opos, uint64_t* __restrict__ oneg, uint32_t cap) {
  __shared__ uint32_t seg[kSegWords];
  load_seg(seg_in, m, seg);
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e >= seg[m] || e >= cap) return;
  uint32_t j = 0;  // the boundaries at or below e: every lane reads the same LDS word
  for (uint32_t i = 1; i < m; ++i) j += seg[i] <= e ? 1u : 0u;
  const uint32_t nb = words[0] < n ? words[0] : n;
  const uint64_t key = hkey[e];
  uint64_t at = 0;
  bool inside;
  const uint32_t lb = runs_before(uniq, nb, P, (int64_t)j - (int64_t)P.first, key, minmax[0],
                                  minmax[1], &at, &inside);
  const bool hit = inside && lb < nb && uniq[lb] == at;
  const uint64_t out = e + before[lb];
  if (out < cap) {
    okey[out] = key;
    opos[out] = hpos[e] + (hit ? cnt[lb] : 0ull);
    oneg[out] = hneg[e] + (hit ? cnt[(size_t)n + lb] : 0ull);
  }
}

inline uint32_t width_of(uint64_t v) {
  uint32_t b = 0;
  for (; v; v >>= 1) ++b;
  return b;
}

}  // namespace
}  // namespace psg

// ------------------------------------------------------------------- host --
using psg::fail;

namespace {

enum RowsBuf {
  R_Y, R_PREDICT, R_WKEY, R_WCNT, R_BKEY, R_KEY_A, R_KEY_B, R_POS_A, R_POS_B, R_COUNTS,
  R_TILE_SUM, R_UNIQ, R_RUN_START, R_RUN_OF, R_CNT, R_RUNKEY, R_LO, R_ISNEW, R_BEFORE, R_COUNT
};

// device words: [0] smallest key of the pass, [1] largest, [2] as two u32:
// runs of the pass, new keys among them; the 256 digit totals; then seg of
// either side of the ping-pong (u32 each)
constexpr size_t kRowsSmallBytes = 3 * 8 + 256 * 4 + 2 * psg::kSegWords * 4;

}  // namespace

struct psg_auc_rows : psg::DeviceBlocks<R_COUNT> {
  int64_t goodness = 0;
  uint32_t m = 1;
  // the table: two sets of key / pos / neg arrays of `cap` entries each
  uint64_t* tab[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  size_t cap = 0;
  int cur = 0;       // the set (and the seg) that holds the table
  size_t bound = 0;  // the resident count, all models, is at most this

  uint32_t* d_words() const { return (uint32_t*)(d_small + 2); }
  uint32_t* d_dtotal() const { return (uint32_t*)(d_small + 3); }
  uint32_t* d_seg(int side) const { return d_dtotal() + 256 + side * psg::kSegWords; }
};

namespace {

using namespace psg;

constexpr size_t kMaxItems = 0xffffffffull;  // positions and ranks are uint32

// seg of the current side, after a wait: seg[m] is the true resident count
int read_seg(psg_auc_rows* h, uint32_t* seg) {
  if (int rc = h->settle()) return rc;
  HIP_TRY(hipMemcpy(seg, h->d_seg(h->cur), 4 * (h->m + 1), hipMemcpyDeviceToHost));
  for (uint32_t j = 0; j < h->m; ++j)
    if (seg[j] > seg[j + 1]) return fail(PSG_ERR_DEVICE, "segment %u ends before it starts", j);
  if (seg[0] != 0 || seg[h->m] > h->cap)
    return fail(PSG_ERR_DEVICE, "%u histogram entries in room for %zu", seg[h->m], h->cap);
  h->bound = seg[h->m];
  return PSG_OK;
}

// Room for `add` more keys, as psg_auc's: the host's bound grows by every
// pass's item count, and the device's count is read only when the bound
// passes the capacity.
int make_room(psg_auc_rows* h, size_t add) {
  if (h->bound + add <= h->cap) return PSG_OK;
  size_t total = 0;
  if (h->cap) {
    uint32_t seg[kSegWords];
    if (int rc = read_seg(h, seg)) return rc;
    total = seg[h->m];
    if (total + add <= h->cap) return PSG_OK;
  }
  if (total + add >= kMaxItems)
    return fail(PSG_ERR_SIZE, "%zu histogram keys >= 2^32 - 1", total + add);
  const size_t cap =
      std::min(kMaxItems, std::max<size_t>({2 * h->cap, total + add, (size_t)1 << 16}));
  uint64_t* fresh[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  for (auto& set : fresh)
    for (auto& p : set)
      if (hipMalloc((void**)&p, 8 * cap) != hipSuccess) {
        (void)hipGetLastError();
        for (auto& set2 : fresh)
          for (auto& q : set2)
            if (q) (void)hipFree(q);
        return fail(PSG_ERR_OOM, "histograms of %zu entries", cap);
      }
  for (int a = 0; a < 3; ++a)
    if (total)
      HIP_TRY(hipMemcpy(fresh[h->cur][a], h->tab[h->cur][a], 8 * total, hipMemcpyDeviceToDevice));
  for (int sd = 0; sd < 2; ++sd)
    for (int a = 0; a < 3; ++a) {
      if (h->tab[sd][a]) (void)hipFree(h->tab[sd][a]);
      h->tab[sd][a] = fresh[sd][a];
    }
  h->cap = cap;
  return PSG_OK;
}

// the blocks of a pass of up to n items
int pass_blocks(psg_auc_rows* h, size_t n_z) {
  const uint32_t ntiles = blocks_of(n_z, kSortTile), nt = blocks_of(n_z, kFlagTile);
  return h->need_all({
      {R_BKEY, 8 * n_z}, {R_KEY_A, 8 * n_z}, {R_KEY_B, 8 * n_z}, {R_POS_A, 4 * n_z},
      {R_POS_B, 4 * n_z}, {R_COUNTS, 4 * 256 * (size_t)ntiles}, {R_TILE_SUM, 4 * (size_t)nt + 4},
      {R_UNIQ, 8 * n_z}, {R_RUN_START, 4 * (n_z + 1)}, {R_RUN_OF, 4 * n_z}, {R_CNT, 16 * n_z},
      {R_RUNKEY, 8 * n_z}, {R_LO, 4 * n_z}, {R_ISNEW, n_z}, {R_BEFORE, 4 * (n_z + 1)}});
}

// One pass of n items (room and blocks are the caller's).  *wide: an
// all-models pass whose composite key does not fit; nothing but the key
// kernel has run then, and the caller takes the models one at a time.
int run_pass(psg_auc_rows* h, uint32_t n, Pass P, const double* y, const double* predict,
             const int64_t* wkey, const uint64_t* weight, int side, hipStream_t s, bool* wide) {
  *wide = false;
  if (int rc = h->order(s)) return rc;
  // (a)
  h->h_small[0] = ~0ull;
  h->h_small[1] = 0;
  HIP_TRY(hipMemcpyAsync(h->d_small, h->h_small, 16, hipMemcpyHostToDevice, s));
  uint64_t* bkey = h->at<uint64_t>(R_BKEY);
  LAUNCH(aucr_keys_kernel, std::min(blocks_of(n, 256), kGridCap), s, predict, wkey,
         (double)h->goodness, n, P, bkey, h->d_small);
  if (int rc = launched("auc rows keys")) return rc;
  // the span decides the composite key's layout and the digits sorted on: the
  // one host wait of an add, as psg_auc's
  HIP_TRY(hipMemcpyAsync(h->h_small, h->d_small, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h->h_small[0] > h->h_small[1]) return fail(PSG_ERR_DEVICE, "auc rows keys: no key range");
  P.b = width_of(h->h_small[1] - h->h_small[0]);
  const uint32_t c = width_of(P.models - 1);  // ceil(log2 models)
  if (P.b + c > 64) {
    *wide = true;
    return h->mark(s);
  }
  const uint64_t differ = P.b + c >= 64 ? ~0ull : (1ull << (P.b + c)) - 1;
  // (b)
  uint64_t* ckey = h->at<uint64_t>(R_KEY_B);
  LAUNCH(aucr_compose_kernel, blocks_of(n, 256), s, bkey, n, P, h->d_small, ckey);
  const SortBuffers sb{h->at<uint64_t>(R_KEY_A), h->at<uint64_t>(R_KEY_B), h->at<uint32_t>(R_POS_A),
                       h->at<uint32_t>(R_POS_B), h->at<uint32_t>(R_COUNTS), h->d_dtotal()};
  const uint64_t* skey = nullptr;
  const uint32_t* spos = nullptr;
  if (int rc = enqueue_radix_sort(ckey, n, differ, sb, &skey, &spos, s)) return rc;
  // (c)
  uint32_t* ts = h->at<uint32_t>(R_TILE_SUM);
  unsigned long long* cnt = h->at<unsigned long long>(R_CNT);
  uint64_t* uniq = h->at<uint64_t>(R_UNIQ);
  const HeadFlag hf{skey};
  const HeadEmit he{skey, uniq, h->at<uint32_t>(R_RUN_START), h->at<uint32_t>(R_RUN_OF)};
  enqueue_flag_scan(hf, he, n, ts, h->d_words(), s);
  HIP_TRY(hipMemsetAsync(cnt, 0, 16 * (size_t)n, s));
  LAUNCH(aucr_run_counts_kernel, blocks_of(n, 256), s, spos, h->at<uint32_t>(R_RUN_OF), y, weight,
         side, n, P.models, cnt);
  // (d)
  const int cur = h->cur, nxt = cur ^ 1;
  const uint32_t cap = (uint32_t)h->cap;
  uint64_t* runkey = h->at<uint64_t>(R_RUNKEY);
  uint32_t* lo_of = h->at<uint32_t>(R_LO);
  uint8_t* isnew = h->at<uint8_t>(R_ISNEW);
  uint32_t* before = h->at<uint32_t>(R_BEFORE);
  LAUNCH(aucr_run_search_kernel, blocks_of(n, 256), s, uniq, h->d_words(), h->d_small,
         h->tab[cur][0], h->d_seg(cur), h->m, P, n, runkey, lo_of, isnew);
  const NewFlag nf{isnew};
  const NewEmit ne{before};
  enqueue_flag_scan(nf, ne, n, ts, h->d_words() + 1, s);
  LAUNCH(aucr_write_new_kernel, blocks_of(n, 256), s, uniq, runkey, lo_of, isnew, before, cnt,
         h->d_words(), n, h->d_seg(cur), h->d_seg(nxt), h->m, P, h->tab[nxt][0], h->tab[nxt][1],
         h->tab[nxt][2], cap);
  if (h->bound)
    LAUNCH(aucr_write_resident_kernel, blocks_of(h->bound, 256), s, h->tab[cur][0], h->tab[cur][1],
           h->tab[cur][2], h->d_seg(cur), h->m, P, uniq, h->d_small, before, cnt, h->d_words(), n,
           h->tab[nxt][0], h->tab[nxt][1], h->tab[nxt][2], cap);
  if (int rc = launched("auc rows add")) return rc;
  h->cur = nxt;
  h->bound += n;
  return h->mark(s);
}

// n examples of m predictions each, device arrays
int add_examples(psg_auc_rows* h, size_t n_z, const double* y, const double* predict,
                 hipStream_t s) {
  if (n_z >= kMaxItems || n_z * h->m >= kMaxItems)
    return fail(PSG_ERR_SIZE, "%zu examples of %u models >= 2^32 - 1 items", n_z, h->m);
  if (n_z == 0) return PSG_OK;
  const size_t items = n_z * h->m;
  if (int rc = make_room(h, items)) return rc;
  if (int rc = pass_blocks(h, items)) return rc;
  bool wide = false;
  if (int rc = run_pass(h, (uint32_t)items, Pass{h->m, 0, 1, 0, 0}, y, predict, nullptr, nullptr, 0,
                        s, &wide))
    return rc;
  for (uint32_t j = 0; wide && j < h->m; ++j) {  // one model: its span always fits
    bool again = false;
    if (int rc = run_pass(h, (uint32_t)n_z, Pass{1, j, h->m, j, 0}, y, predict, nullptr, nullptr, 0,
                          s, &again))
      return rc;
  }
  return PSG_OK;
}

// model j's segment as the AUCData of auc.h:85-97, after a wait
int export_lists(psg_auc_rows* h, uint32_t j, std::vector<int64_t>* tk, std::vector<uint64_t>* tc,
                 std::vector<int64_t>* fk, std::vector<uint64_t>* fc) {
  HIP_TRY(hipSetDevice(h->device));
  uint32_t seg[kSegWords] = {0};
  if (h->cap)
    if (int rc = read_seg(h, seg)) return rc;
  const size_t at = seg[j], len = seg[j + 1] - seg[j];
  try {
    std::vector<uint64_t> key(len), pos(len), neg(len);
    if (len) {
      HIP_TRY(hipMemcpy(key.data(), h->tab[h->cur][0] + at, 8 * len, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(pos.data(), h->tab[h->cur][1] + at, 8 * len, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(neg.data(), h->tab[h->cur][2] + at, 8 * len, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < len; ++i) {
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

int psg_auc_rows_create(psg_ctx* ctx, int64_t goodness, int m, psg_auc_rows** out) {
  if (!ctx || !out) return fail(PSG_ERR_ARG, "null argument");
  *out = nullptr;
  if (m < 1 || m > PSG_FTRL_MAX_MODELS)
    return fail(PSG_ERR_ARG, "%d models: 1 .. %d", m, PSG_FTRL_MAX_MODELS);
  int device, dtype;
  hipStream_t stream;
  psg::ctx_info(ctx, &device, &dtype, &stream);
  HIP_TRY(hipSetDevice(device));
  psg_auc_rows* h = new (std::nothrow) psg_auc_rows();
  if (!h) return fail(PSG_ERR_OOM, "host allocation");
  h->goodness = goodness;
  h->m = (uint32_t)m;
  if (!h->open(ctx, kRowsSmallBytes) ||
      hipMemset(h->d_small, 0, kRowsSmallBytes) != hipSuccess) {
    (void)hipGetLastError();
    psg_auc_rows_destroy(h);
    return fail(PSG_ERR_OOM, "auc rows control blocks");
  }
  *out = h;
  return PSG_OK;
}

void psg_auc_rows_destroy(psg_auc_rows* h) {
  if (!h) return;
  h->close();
  for (auto& set : h->tab)
    for (auto& p : set)
      if (p) (void)hipFree(p);
  delete h;
}

int psg_auc_rows_clear(psg_auc_rows* h) {
  if (!h) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (int rc = h->order(s)) return rc;
  HIP_TRY(hipMemsetAsync(h->d_seg(0), 0, 2 * kSegWords * 4, s));
  h->bound = 0;
  return h->mark(s);
}

int psg_auc_rows_set_goodness(psg_auc_rows* h, int64_t goodness) {
  if (!h) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  uint32_t seg[kSegWords] = {0};
  if (h->bound && h->cap)
    if (int rc = read_seg(h, seg)) return rc;
  if (seg[h->m])
    return fail(PSG_ERR_ARG, "psg_auc_rows_set_goodness on histograms of %u keys", seg[h->m]);
  h->goodness = goodness;
  return PSG_OK;
}

int psg_auc_rows_add_dev(psg_auc_rows* h, const double* y_dev, const double* predict_dev, size_t n,
                         void* stream) {
  if (!h || (n && (!y_dev || !predict_dev))) return fail(PSG_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  return add_examples(h, n, y_dev, predict_dev, h->pick(stream));
}

int psg_auc_rows_add(psg_auc_rows* h, const double* y, const double* predict, size_t n) {
  if (!h || (n && (!y || !predict))) return fail(PSG_ERR_ARG, "null argument");
  if (n >= kMaxItems || n * h->m >= kMaxItems)
    return fail(PSG_ERR_SIZE, "%zu examples of %u models >= 2^32 - 1 items", n, h->m);
  if (n == 0) return PSG_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (int rc = h->settle()) return rc;  // the staging blocks may be in use
  if (int rc = h->need(R_Y, 8 * n)) return rc;
  if (int rc = h->need(R_PREDICT, 8 * n * h->m)) return rc;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(h->b[R_Y].p, y, 8 * n, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(h->b[R_PREDICT].p, predict, 8 * n * h->m, hipMemcpyHostToDevice, s));
  return add_examples(h, n, h->at<double>(R_Y), h->at<double>(R_PREDICT), s);
}

int psg_auc_rows_merge(psg_auc_rows* h, int j, const int64_t* tp_key, const uint64_t* tp_count,
                       size_t ntp, const int64_t* fp_key, const uint64_t* fp_count, size_t nfp) {
  if (!h || (ntp && (!tp_key || !tp_count)) || (nfp && (!fp_key || !fp_count)))
    return fail(PSG_ERR_ARG, "null argument");
  if (j < 0 || (uint32_t)j >= h->m) return fail(PSG_ERR_ARG, "model %d of %u", j, h->m);
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
    if (int rc = h->need(R_WKEY, 8 * k.size())) return rc;
    if (int rc = h->need(R_WCNT, 8 * k.size())) return rc;
    HIP_TRY(hipMemcpy(h->b[R_WKEY].p, k.data(), 8 * k.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->b[R_WCNT].p, c.data(), 8 * c.size(), hipMemcpyHostToDevice));
    if (int rc = make_room(h, k.size())) return rc;
    if (int rc = pass_blocks(h, k.size())) return rc;
    bool wide = false;  // never: one model
    if (int rc = run_pass(h, (uint32_t)k.size(), Pass{1, (uint32_t)j, 1, 0, 0}, nullptr, nullptr,
                          h->at<int64_t>(R_WKEY), h->at<uint64_t>(R_WCNT), side, s, &wide))
      return rc;
  }
  return PSG_OK;
}

int psg_auc_rows_data(psg_auc_rows* h, int j, int64_t* tp_key, uint64_t* tp_count, size_t tp_cap,
                      size_t* ntp, int64_t* fp_key, uint64_t* fp_count, size_t fp_cap,
                      size_t* nfp) {
  if (!h || !ntp || !nfp) return fail(PSG_ERR_ARG, "null argument");
  *ntp = *nfp = 0;
  if (j < 0 || (uint32_t)j >= h->m) return fail(PSG_ERR_ARG, "model %d of %u", j, h->m);
  std::vector<int64_t> tk, fk;
  std::vector<uint64_t> tc, fc;
  if (int rc = export_lists(h, (uint32_t)j, &tk, &tc, &fk, &fc)) return rc;
  *ntp = tk.size();
  *nfp = fk.size();
  if (tk.size() > tp_cap || fk.size() > fp_cap)
    return fail(PSG_ERR_SIZE, "psg_auc_rows_data: %zu + %zu entries, room for %zu + %zu",
                tk.size(), fk.size(), tp_cap, fp_cap);
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

int psg_auc_rows_accuracy(psg_auc_rows* h, double threshold, double* v) {
  if (!h || !v) return fail(PSG_ERR_ARG, "null argument");
  for (uint32_t j = 0; j < h->m; ++j) {
    std::vector<int64_t> tk, fk;
    std::vector<uint64_t> tc, fc;
    if (int rc = export_lists(h, j, &tk, &tc, &fk, &fc)) return rc;
    if (int rc = psg_auc_accuracy_data(h->goodness, tk.data(), tc.data(), tk.size(), fk.data(),
                                       fc.data(), fk.size(), threshold, v + j))
      return rc;
  }
  return PSG_OK;
}

int psg_auc_rows_evaluate(psg_auc_rows* h, int mode, double* v) {
  if (!h || !v) return fail(PSG_ERR_ARG, "null argument");
  for (uint32_t j = 0; j < h->m; ++j) {
    std::vector<int64_t> tk, fk;
    std::vector<uint64_t> tc, fc;
    if (int rc = export_lists(h, j, &tk, &tc, &fk, &fc)) return rc;
    if (int rc = psg_auc_evaluate_data(tk.data(), tc.data(), tk.size(), fk.data(), fc.data(),
                                       fk.size(), mode, v + j))
      return rc;
  }
  return PSG_OK;
}

}  // extern "C"
