// psg_terafea.hip -- the row sort of the TERAFEA ingest:
// ExampleParser::parseTerafea's std::sort of every line's keys
// (src/data/example_parser.cc:198), its group split (key >> 54), the feature
// id shuffle (:205-209) and the beta entry (:220-230), over the raw keys the
// tokeniser of psg_text.hip left in line order.
//
// The sort is segmented: rows of 0 to ~20 K keys, most of them short.  The
// work is divided by entries, never by rows:
//
//  (1) check_kernel: a key below 2^54 (group 0) rejects its line, before any
//      key moves.
//  (2) tile_kernel: a workgroup of 256 lanes takes kTile = 1024 consecutive
//      entries, 4 per lane, whatever rows they belong to.  A lane finds the
//      row of its first entry by one search of offset[] and searches again
//      only where its 4 entries cross into another row; the row is the
//      entry's tag.  The tile is sorted by (tag, key) with a bitonic network:
//      tags never decrease along the entries, so every row's keys come out
//      sorted where the row lies, and many short rows share one workgroup.
//      Steps of distance 2 and 1 are compare-exchanges between a lane's own
//      registers; steps of distance 4 .. 512 go through LDS (keys 8 KB,
//      tags 4 KB), two pairs per lane and step.  The piece of a row that a
//      tile's edge cuts off comes out sorted as a piece.
//  (3) edge_kernel, cut rows: a row of at most kTile entries crosses at most
//      one tile edge and is then two sorted runs.  The workgroup of that edge
//      loads the first run ascending and the second descending around a pad
//      of +inf, which is one bitonic sequence, and runs the network's last
//      phase (log2 kTile steps) over it.
//  (4) edge_kernel, long rows: a row of more than kTile entries is sorted by
//      the workgroup of the first tile edge inside it, in place in global
//      memory, by the same network in its one-direction form over the next
//      power of two (entries past the row's end are a virtual +inf that never
//      moves).  A token and its separator are two bytes or more, so a line
//      of at most 61438 bytes holds fewer than 32768 keys ("-1", which
//      strtoull takes for 2^64 - 1, gives about 20 K valid ones): a longer
//      row belongs to a line the length rule rejects and is left alone.
//      Correct, rare in CTR data and not tuned.
//  (5) finish_kernel: one lane per sorted key writes index (the key, or its
//      murmur shuffle) and slot = key >> 54, at e + row with the beta entry,
//      which the lanes past the keys append per row; shift_kernel then moves
//      offset[r] by r.
// No kernel takes a list from the host or hands one back: which rows are cut
// or long is read from offset[] by the workgroup of the tile edge.  Every
// loop's trip count is fixed by kTile, by 32 (the searches) or by the 32768
// bound, never by the keys.  No atomics but the minimum over rejected lines:
// the same text gives the same arrays on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psg.h"
#include "psg_host.h"
#include "psg_minibatch.h"
#include "psg_sort.h"  // LAUNCH, blocks_of, launched
#include "psg_text.h"

namespace psg {
namespace {

constexpr uint32_t kTile = 1024;     // entries per workgroup
constexpr uint32_t kPer = 4;         // entries per lane: kTile / 256
constexpr uint32_t kLongMax = 32768;  // a line under kMaxLine bytes holds fewer tokens
static_assert(kLongMax >= text::kMaxLine / 2, "a token and its separator are two bytes");
constexpr uint32_t kPadTag = 0xffffffffu;

// the row that holds entry j < offset[rows]: the last one with offset[row] <= j
__device__ __forceinline__ uint32_t row_holding(const uint64_t* __restrict__ offset, uint32_t rows,
                                                uint64_t j) {
  uint32_t lo = 0, hi = rows;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (offset[mid] <= j) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

struct Item {
  uint64_t key;
  uint32_t tag;
};
__device__ __forceinline__ bool before(const Item& a, const Item& b) {
  return a.tag < b.tag || (a.tag == b.tag && a.key < b.key);
}
// a stays below b when `up`, above it otherwise
__device__ __forceinline__ void cmpx(Item& a, Item& b, bool up) {
  if (before(b, a) == up) {
    const Item t = a;
    a = b;
    b = t;
  }
}

// The steps of distance min(kPer, k) / 2 .. 1 of phase k over the lane's own
// elements, the first of which is element `base` of the tile.
__device__ __forceinline__ void reg_steps(Item (&it)[kPer], uint32_t base, uint32_t k) {
#pragma unroll
  for (uint32_t j = kPer / 2; j >= 1; j >>= 1) {
    if (j >= k) continue;
#pragma unroll
    for (uint32_t a = 0; a < kPer; ++a)
      if ((a & j) == 0) cmpx(it[a], it[a | j], ((base + a) & k) == 0);
  }
}

// Phase k >= 2 * kPer of the network over the tile: the lane's elements
// through LDS for the steps of distance k / 2 .. kPer, then back for the
// rest.  Every lane of the workgroup comes here.
__device__ __forceinline__ void lds_phase(Item (&it)[kPer], uint32_t k, uint64_t* s_key,
                                          uint32_t* s_tag) {
  const uint32_t base = threadIdx.x * kPer;
#pragma unroll
  for (uint32_t a = 0; a < kPer; ++a) {
    s_key[base + a] = it[a].key;
    s_tag[base + a] = it[a].tag;
  }
  __syncthreads();
  for (uint32_t j = k >> 1; j >= kPer; j >>= 1) {
#pragma unroll
    for (uint32_t q = 0; q < kTile / 512; ++q) {
      const uint32_t t = threadIdx.x + 256u * q;
      const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
      Item x{s_key[i], s_tag[i]}, y{s_key[l], s_tag[l]};
      if (before(y, x) == ((i & k) == 0)) {
        s_key[i] = y.key;
        s_tag[i] = y.tag;
        s_key[l] = x.key;
        s_tag[l] = x.tag;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (uint32_t a = 0; a < kPer; ++a) it[a] = Item{s_key[base + a], s_tag[base + a]};
  reg_steps(it, base, k);
}

// ---- (1) ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void check_kernel(const uint64_t* __restrict__ raw,
                                                    const uint64_t* __restrict__ offset,
                                                    uint32_t rows, uint32_t n,
                                                    uint32_t* __restrict__ bad) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= n || (raw[j] >> text::kGroupShift) != 0) return;
  atomicMin(bad, row_holding(offset, rows, j));
}

// ---- (2) ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void tile_kernel(uint64_t* __restrict__ raw,
                                                   const uint64_t* __restrict__ offset,
                                                   uint32_t rows, uint32_t n) {
  __shared__ uint64_t s_key[kTile];
  __shared__ uint32_t s_tag[kTile];
  const uint32_t base = threadIdx.x * kPer;
  const uint64_t e0 = (uint64_t)blockIdx.x * kTile + base;
  Item it[kPer];
  if (e0 + kPer <= n) {  // 16-byte loads
    const ulonglong2* p = (const ulonglong2*)(raw + e0);
#pragma unroll
    for (uint32_t a = 0; a < kPer; a += 2) {
      const ulonglong2 v = p[a / 2];
      it[a].key = v.x;
      it[a + 1].key = v.y;
    }
  } else {
#pragma unroll
    for (uint32_t a = 0; a < kPer; ++a) it[a].key = e0 + a < n ? raw[e0 + a] : ~0ull;
  }
  uint32_t r = 0;
  uint64_t end = 0;  // the first entry past row r
#pragma unroll
  for (uint32_t a = 0; a < kPer; ++a) {
    const uint64_t e = e0 + a;
    if (e >= n) {
      it[a].tag = kPadTag;  // rows < 2^32 - 1: past every row
      continue;
    }
    if (e >= end) {
      r = row_holding(offset, rows, e);
      end = offset[r + 1];
    }
    it[a].tag = r;
  }
#pragma unroll
  for (uint32_t k = 2; k <= kPer; k <<= 1) reg_steps(it, base, k);
  for (uint32_t k = 2 * kPer; k <= kTile; k <<= 1) lds_phase(it, k, s_key, s_tag);
#pragma unroll
  for (uint32_t a = 0; a < kPer; ++a)
    if (e0 + a < n) raw[e0 + a] = it[a].key;
}

// ---- (3), (4) -------------------------------------------------------------------
// Workgroup b stands at the tile edge p = b * kTile and looks at the row that
// holds entry p.
template <bool kLong>
__global__ __launch_bounds__(256) void edge_kernel(uint64_t* __restrict__ raw,
                                                   const uint64_t* __restrict__ offset,
                                                   uint32_t rows, uint32_t n) {
  __shared__ uint64_t s_key[kLong ? 1 : kTile];
  __shared__ uint32_t s_tag[kLong ? 1 : kTile];
  const uint64_t p = (uint64_t)blockIdx.x * kTile;
  if (p >= n) return;
  const uint32_t r = row_holding(offset, rows, p);
  const uint64_t s0 = offset[r], s1 = offset[r + 1];
  if (s0 > p || s1 <= p || s1 > n) return;  // never, by the tokeniser's offsets
  const uint64_t len64 = s1 - s0;
  if (!kLong) {
    if (s0 == p || len64 > kTile) return;  // the row starts at the edge, or is long
    const uint32_t la = (uint32_t)(p - s0), lb = (uint32_t)(s1 - p), len = la + lb;
    const uint32_t base = threadIdx.x * kPer;
    Item it[kPer];
#pragma unroll
    for (uint32_t a = 0; a < kPer; ++a) {
      const uint32_t i = base + a;
      if (i < la)
        it[a] = Item{raw[s0 + i], 0u};
      else if (i >= kTile - lb)
        it[a] = Item{raw[p + (kTile - 1 - i)], 0u};  // the second run, descending
      else
        it[a] = Item{~0ull, 1u};  // above every key
    }
    lds_phase(it, kTile, s_key, s_tag);
#pragma unroll
    for (uint32_t a = 0; a < kPer; ++a)
      if (base + a < len) raw[s0 + base + a] = it[a].key;
  } else {
    // the first edge at or after the row's start sorts it
    if (len64 <= kTile || p - s0 >= kTile || len64 > kLongMax) return;
    const uint32_t len = (uint32_t)len64;
    uint64_t* k = raw + s0;
    uint32_t npow = kTile;
    while (npow < len) npow <<= 1;  // <= kLongMax
    const auto step = [&](uint32_t i, uint32_t l) {
      if (l < len) {  // an element past the row is +inf and stays
        const uint64_t x = k[i], y = k[l];
        if (y < x) {
          k[i] = y;
          k[l] = x;
        }
      }
    };
    for (uint32_t span = 2; span <= npow; span <<= 1) {
      const uint32_t half = span >> 1;
      for (uint32_t t = threadIdx.x; t < npow / 2; t += 256) {  // the flip: i with span - 1 - i
        const uint32_t start = (t & ~(half - 1)) << 1, in = t & (half - 1);
        step(start + in, start + span - 1 - in);
      }
      __syncthreads();
      for (uint32_t j = half >> 1; j >= 1; j >>= 1) {
        for (uint32_t t = threadIdx.x; t < npow / 2; t += 256) {
          const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          step(i, i + j);
        }
        __syncthreads();
      }
    }
  }
}

// ---- (5) ----------------------------------------------------------------------
// Lanes [0, n): the sorted keys.  Lanes [n, n + rows) with beta: row g - n's
// last entry.  offset[] is still the tokeniser's.
__global__ __launch_bounds__(256) void finish_kernel(const uint64_t* __restrict__ raw,
                                                     const uint64_t* __restrict__ offset,
                                                     uint32_t rows, uint32_t n, int shuffle,
                                                     int beta, uint64_t* __restrict__ index,
                                                     uint16_t* __restrict__ slot) {
  const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (g < n) {
    const uint64_t key = raw[g];
    const uint64_t dst = beta ? g + row_holding(offset, rows, g) : g;
    index[dst] = shuffle ? text::murmur_shuffle(key) : key;
    slot[dst] = (uint16_t)(key >> text::kGroupShift);
  } else if (beta && g - n < rows) {
    const uint64_t r = g - n, dst = offset[r + 1] + r;
    index[dst] = 0;
    slot[dst] = text::kBetaSlot;
  }
}

// with beta: offset[r] += r, and the entries kept grow by the rows kept
__global__ __launch_bounds__(256) void shift_kernel(uint64_t* __restrict__ offset, uint32_t rows,
                                                    const uint32_t* __restrict__ rows_kept,
                                                    uint32_t* __restrict__ nnz_kept) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r <= rows) offset[r] += r;
  if (r == 0) *nnz_kept += *rows_kept;
}

}  // namespace

int terafea_check(const uint64_t* raw, const uint64_t* offset, uint32_t rows, uint32_t n,
                  uint32_t* bad, hipStream_t s) {
  if (!n) return PSG_OK;
  LAUNCH(check_kernel, blocks_of(n, 256), s, raw, offset, rows, n, bad);
  return launched("terafea check");
}

int terafea_sort(uint64_t* raw, const uint64_t* offset, uint32_t rows, uint32_t n,
                 hipStream_t s) {
  if (n < 2) return PSG_OK;
  const uint32_t nt = blocks_of(n, kTile);
  LAUNCH(tile_kernel, nt, s, raw, offset, rows, n);
  if (nt > 1) {
    LAUNCH(edge_kernel<false>, nt, s, raw, offset, rows, n);
    LAUNCH(edge_kernel<true>, nt, s, raw, offset, rows, n);
  }
  return launched("terafea sort");
}

int terafea_finish(const uint64_t* raw, uint64_t* offset, uint32_t rows, uint32_t n,
                   unsigned flags, uint64_t* index, uint16_t* slot, const uint32_t* rows_kept,
                   uint32_t* nnz_kept, hipStream_t s) {
  const int beta = (flags & PSG_TERAFEA_BETA) != 0;
  const uint64_t lanes = (uint64_t)n + (beta ? rows : 0u);
  if (lanes)
    LAUNCH(finish_kernel, blocks_of(lanes, 256), s, raw, offset, rows, n,
           (int)((flags & PSG_TERAFEA_SHUFFLE) != 0), beta, index, slot);
  if (beta) LAUNCH(shift_kernel, blocks_of((uint64_t)rows + 1, 256), s, offset, rows, rows_kept,
                   nnz_kept);
  return launched("terafea finish");
}

}  // namespace psg

extern "C" size_t psg_terafea_tile(void) { return psg::kTile; }
