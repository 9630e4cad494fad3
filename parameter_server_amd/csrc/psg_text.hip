// psg_text.hip -- text in, resident minibatch out:
// StreamReader::readMatricesFromText (src/data/stream_reader.h:50-122) over
// ExampleParser::parseLibsvm / parseAdfea (src/data/example_parser.cc:84-160)
// as kernels over the bytes of the text, and psg_mb_load_text.
//
// The work is divided by bytes: a workgroup takes one chunk of kChunk bytes,
// a lane 16 consecutive bytes of it (one 16-byte load, the wave's loads
// coalesced), and classifies them in registers: newline, delimiter, token
// start (a token byte after a delimiter, a newline or the start of the text).
// What a byte means depends on three things before it, which are carried
// across lanes and chunks by scans: the line it is in (newlines before it),
// the ordinal of its token within the line (token starts since the last
// newline) and whether a token is open (the byte before it: one byte of
// halo).  The lane that owns a token's first byte reads the token to its end,
// across the chunk's boundary where needed.
//
//  (1) count_kernel: per chunk, its newlines, its token starts, and the token
//      starts after its last newline.
//  (2) chunk_scan_kernel (one workgroup): the line and the token ordinal at
//      every chunk's first byte; the lines taken (max_rows, `final`).
//  (3) class_kernel: per lane and per chunk, the entries (matrix positions)
//      and the slow tokens among the lines taken; the fast grammar of
//      psg_text.h decides what is slow.
//  (4) row_scan_kernel (psg_sort.h) over the chunks' two counts: every
//      chunk's first entry and first slow token, and the totals.  The host
//      reads the sizes and sizes the minibatch's blocks.
//  (5) emit_kernel: offset at every line's first byte, index / value / y of
//      the fast tokens straight into the minibatch's blocks, the slow tokens
//      into their list, each line's end, and the lines rejected on sight
//      (no token, too few tokens, a NUL, a pair without ':').
//  (6) with slow tokens: the host runs them through libc
//      (psg::text::resolve_slow) and patch_kernel writes the results or
//      rejects their lines.
//  (7) order_kernel (LIBSVM: idx must not decrease within a line),
//      line_kernel (the length limit), verdict_kernel (the first rejected
//      line, the rows and entries kept, the bytes consumed).
// psg_mb_load_text_groups is the same pipeline in its grouped
// mode: FileLineReader's line rule for ADFEA (`ga`: the line's '\n' and the
// '\r' chopped with it are no token bytes, lane_tok_start), the slot id of
// every entry into a uint16 block, slow slot tokens through (6), and after (7)
// the OR / AND of the ids kept (slot_bits_kernel) for the grouping's sort.
// Integer atomics: the minimum over the rejected lines, nothing else.  Every
// array element has one writer (or, for a slow token, a second one ordered
// after the first), so the same text gives the same arrays on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/psg.h"
#include "psg_host.h"
#include "psg_minibatch.h"
#include "psg_sort.h"
#include "psg_text.h"

namespace psg {
namespace {

using namespace psg::text;

constexpr uint32_t kChunk = 4096;  // bytes per workgroup: 256 lanes x 16
constexpr uint32_t kNone = 0xffffffffu;

// control words (uint32) on the device
enum Word {
  W_LINES = 0, W_ROWS, W_NNZ, W_SLOW, W_BAD, W_ROWS_OUT, W_NNZ_OUT, W_CONSUMED,
  W_SLOT_OR, W_SLOT_AND,  // the grouped parse: over the slot ids of the entries kept
  W_COUNT
};

// per-chunk arrays, each `nc` words, in one block
struct Chunks {
  uint32_t *nl, *tok, *after;      // (1)
  uint32_t *line_base, *ord_base;  // (2)
  uint32_t *feat, *slow;           // (3) counts, then (4) their exclusive scans; adjacent
};

__host__ __device__ inline Chunks chunks_of(uint32_t* p, uint32_t nc) {
  return Chunks{p, p + nc, p + 2 * (size_t)nc, p + 3 * (size_t)nc, p + 4 * (size_t)nc,
                p + 5 * (size_t)nc, p + 6 * (size_t)nc};
}

// The lane's 16 bytes (those past the text are not looked at) and the byte
// before them ('\n' before the text: a line starts there).
struct Lane {
  uint64_t lo, hi;  // bytes 0..7 and 8..15 (no array: the walk indexes them by a loop counter)
  __device__ __forceinline__ unsigned char at(uint32_t j) const {
    return (unsigned char)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 255u);
  }
  unsigned char prev;
  unsigned char next;  // the byte after them (0 past the text): the grouped parse's look-ahead
  uint32_t n;   // how many of the 16 are text
  uint64_t i0;  // the first one's place
};

__device__ __forceinline__ Lane load_lane(const unsigned char* __restrict__ text, uint64_t nbytes) {
  Lane l;
  l.i0 = (uint64_t)blockIdx.x * kChunk + threadIdx.x * 16u;
  l.n = l.i0 < nbytes ? (uint32_t)(nbytes - l.i0 < 16 ? nbytes - l.i0 : 16) : 0u;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (l.n) v = *(const uint4*)(text + l.i0);  // the block is padded to a whole chunk
  l.lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
  l.hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
  l.prev = l.n && l.i0 ? text[l.i0 - 1] : '\n';
  l.next = l.n && l.i0 + l.n < nbytes ? text[l.i0 + l.n] : 0;
  return l;
}

__device__ __forceinline__ bool tok_start(int libsvm, unsigned char prev, unsigned char c) {
  return !is_delim(libsvm, c) && (prev == '\n' || is_delim(libsvm, prev));
}
// Byte j of the lane starts a token.  ga (grouped ADFEA): the line's '\n' and
// the '\r' chopped with it are no token bytes, which takes the byte after c.
// A chopped '\r' is never the byte before a token byte (a '\n' or the end of
// the text follows it), so `prev` needs no look-ahead of its own.
__device__ __forceinline__ bool lane_tok_start(const Lane& l, int libsvm, int ga, uint32_t j,
                                               unsigned char prev, unsigned char c,
                                               uint64_t nbytes) {
  if (!ga) return tok_start(libsvm, prev, c);
  const unsigned char next = j + 1 < l.n ? l.at(j + 1) : l.next;
  return !grouped_gap(c, next, l.i0 + j + 1 == nbytes) && (prev == '\n' || is_delim(0, prev));
}

// the lane's newlines, token starts, and token starts after its last newline
__device__ __forceinline__ void lane_counts(const Lane& l, int libsvm, int ga, uint64_t nbytes,
                                            uint32_t* nls, uint32_t* total, uint32_t* after) {
  uint32_t n = 0, t = 0, a = 0;
  unsigned char prev = l.prev;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if ((uint32_t)j < l.n) {
      const unsigned char c = l.at(j);
      const uint32_t st = lane_tok_start(l, libsvm, ga, (uint32_t)j, prev, c, nbytes) ? 1u : 0u;
      t += st;
      a += st;  // an ADFEA '\n' that starts a token belongs to the line it ends
      if (c == '\n') {
        ++n;
        a = 0;
      }
      prev = c;
    }
  }
  *nls = n;
  *total = t;
  *after = a;
}

// The line and the token ordinal at the lane's first byte.  With P the token
// starts of the chunk before the lane, a lane that holds a newline hands
// G = after - (P + total) to the lanes behind it, up to the next such lane:
// their ordinal is P + G.  Before the chunk's first newline G is the chunk's
// ordinal base.  sh: 16 LDS words.  Every lane of the workgroup comes here.
__device__ __forceinline__ void lane_state(uint32_t nls, uint32_t total, uint32_t after,
                                           uint32_t line_base, uint32_t ord_base, uint32_t* sh,
                                           uint32_t* line0, uint32_t* ord0) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t tot;
  const uint32_t exl = block_exscan(nls, sh, &tot);
  const uint32_t p = block_exscan(total, sh + 4, &tot);
  const uint32_t g = after - (p + total);
  const uint64_t m = __ballot(nls != 0);
  const int top = m ? 63 - __clzll((long long)m) : 0;
  const uint32_t gtop = __shfl(g, top, 64);
  if (lane == 0) {
    sh[8 + w] = m ? 1u : 0u;
    sh[12 + w] = gtop;
  }
  __syncthreads();
  uint32_t carry = ord_base;
  for (uint32_t i = 0; i < w; ++i)
    if (sh[8 + i]) carry = sh[12 + i];
  const uint64_t lower = m & ((1ull << lane) - 1);
  const int src = lower ? 63 - __clzll((long long)lower) : 0;
  const uint32_t gsrc = __shfl(g, src, 64);
  *line0 = line_base + exl;
  *ord0 = p + (lower ? gsrc : carry);
  __syncthreads();  // sh is free again
}

// ---- (1) ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void count_kernel(const unsigned char* __restrict__ text,
                                                    uint64_t nbytes, int libsvm, int ga,
                                                    Chunks ch) {
  __shared__ uint32_t sh[16];
  const Lane l = load_lane(text, nbytes);
  uint32_t nls, total, after;
  lane_counts(l, libsvm, ga, nbytes, &nls, &total, &after);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t m = __ballot(nls != 0);
  if (lane == 0) sh[8 + w] = m ? (w * 64u + 63u - (uint32_t)__clzll((long long)m)) + 1u : 0u;
  __syncthreads();
  uint32_t last = 0;  // 1 + the last lane of the workgroup that holds a newline; 0: none
  for (uint32_t i = 0; i < 4; ++i) last = sh[8 + i] > last ? sh[8 + i] : last;
  const uint32_t t = threadIdx.x + 1u;
  const uint32_t a = t > last ? total : (t == last ? after : 0u);
  uint32_t nl_sum, tok_sum, after_sum;
  (void)block_exscan(nls, sh, &nl_sum);
  (void)block_exscan(total, sh + 4, &tok_sum);
  (void)block_exscan(a, sh, &after_sum);
  if (threadIdx.x == 0) {
    ch.nl[blockIdx.x] = nl_sum;
    ch.tok[blockIdx.x] = tok_sum;
    ch.after[blockIdx.x] = after_sum;
  }
}

// ---- (2) ----------------------------------------------------------------------
// One workgroup.  Lane t takes the chunks [t * per, (t + 1) * per): their sum
// first, lane 0 walks the 256 sums, then every lane walks its chunks again
// with its carry.
__global__ __launch_bounds__(256) void chunk_scan_kernel(const unsigned char* __restrict__ text,
                                                         uint64_t nbytes, uint32_t nc, Chunks ch,
                                                         uint32_t max_rows, int final,
                                                         uint32_t* __restrict__ words) {
  __shared__ uint32_t s_nl[256], s_ord[256], s_has[256];
  const uint32_t per = (nc + 255u) / 256u;
  const uint32_t b = threadIdx.x * per < nc ? threadIdx.x * per : nc;
  const uint32_t e = b + per < nc ? b + per : nc;
  uint32_t nl = 0, ord = 0, has = 0;  // ord: the token starts since the span's last newline
  for (uint32_t c = b; c < e; ++c) {
    nl += ch.nl[c];
    if (ch.nl[c]) {
      has = 1;
      ord = ch.after[c];
    } else {
      ord += ch.tok[c];
    }
  }
  s_nl[threadIdx.x] = nl;
  s_ord[threadIdx.x] = ord;
  s_has[threadIdx.x] = has;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t ln = 0, od = 0;
    for (uint32_t t = 0; t < 256; ++t) {
      const uint32_t n = s_nl[t], o = s_ord[t], h = s_has[t];
      s_nl[t] = ln;
      s_ord[t] = od;
      ln += n;
      od = h ? o : od + o;
    }
    const bool partial = final && nbytes && text[nbytes - 1] != '\n';
    const uint32_t lines = ln + (partial ? 1u : 0u);
    words[W_LINES] = lines;
    words[W_ROWS] = lines < max_rows ? lines : max_rows;
  }
  __syncthreads();
  nl = s_nl[threadIdx.x];
  ord = s_ord[threadIdx.x];
  for (uint32_t c = b; c < e; ++c) {
    ch.line_base[c] = nl;
    ch.ord_base[c] = ord;
    nl += ch.nl[c];
    ord = ch.nl[c] ? ch.after[c] : ord + ch.tok[c];
  }
}

// ---- (3), (5) -------------------------------------------------------------------
struct Emit {  // (5)'s outputs; all null in (3)
  uint64_t* offset;
  uint64_t* index;
  double* value;
  double* y;
  uint16_t* slot;  // the grouped parse; null otherwise
  uint32_t* line_end;
  SlowToken* slow;
  uint32_t* words;
  uint32_t nnz;    // the entries of the lines taken
  uint32_t nslow;  // ... and their slow tokens
};

// The lane's walk over its bytes.  kEmit false: counts the entries and slow
// tokens that start in the lane, among lines below `rows`.  kEmit true: the
// same walk with the lane's first entry `fpos` and first slow token `spos`.
template <bool kEmit>
__device__ __forceinline__ void lane_walk(const unsigned char* __restrict__ text, uint64_t nbytes,
                                          int libsvm, int ga, int final, const Lane& l,
                                          uint32_t line0,
                                          uint32_t ord0, uint32_t rows, uint32_t fpos,
                                          uint32_t spos, const Emit& o, uint32_t* nfeat,
                                          uint32_t* nslow) {
  // The lane's newlines, token starts and NULs as bit masks first, then one
  // loop over the token starts: the lanes of a wave convert their k-th token
  // together, whatever byte it starts at.
  uint32_t nlm = 0, stm = 0, zero = 0;
  unsigned char prev = l.prev;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if ((uint32_t)j < l.n) {
      const unsigned char c = l.at(j);
      if (c == '\n') nlm |= 1u << j;
      if (c == 0) zero |= 1u << j;
      if (lane_tok_start(l, libsvm, ga, (uint32_t)j, prev, c, nbytes)) stm |= 1u << j;
      prev = c;
    }
  }
  const auto line_at = [&](uint32_t j) { return line0 + (uint32_t)__popc(nlm & ((1u << j) - 1)); };
  // the token starts of byte j's line before byte j (an ADFEA '\n' that starts
  // a token belongs to the line it ends)
  const auto ord_at = [&](uint32_t j) {
    const uint32_t below = (1u << j) - 1, nb = nlm & below;
    if (!nb) return ord0 + (uint32_t)__popc(stm & below);
    const uint32_t last = 31u - (uint32_t)__clz((int)nb);
    return (uint32_t)__popc(stm & below & ~((2u << last) - 1));
  };
  uint32_t feat = 0, slow = 0, featm = 0;  // featm: the starts that are entries
  for (uint32_t m = stm; m; m &= m - 1) {
    const uint32_t j = (uint32_t)__ffs((int)m) - 1;
    const uint32_t line = line_at(j), ord = ord_at(j);
    if (line >= rows) break;  // and so is every later token's
    const uint64_t i = l.i0 + j;
    const unsigned char* p = text + i;
    const size_t avail = (size_t)(nbytes - i);
    int verdict = kFast, kind = -1;
    uint32_t dest = kNone;
    uint64_t key = 0;
    double val = 0.0;
    if (libsvm) {
      float f = 0.0f;
      if (ord == 0) {
        verdict = libsvm_label(p, avail, &f);
        kind = kLibsvmLabel;
        dest = line;
      } else {
        verdict = libsvm_pair(p, avail, &key, &f);
        kind = kLibsvmPair;
        dest = fpos + feat;
        if (kEmit && o.slot && dest < o.nnz) o.slot[dest] = 1;  // parseLibsvm's one slot
        ++feat;
        featm |= 1u << j;
      }
      val = (double)f;
    } else if (ord == 2) {
      verdict = ga ? grouped_label(p, avail, &val) : adfea_label(p, avail, &val);
      kind = kAdfeaLabel;
      dest = line;
    } else if (ord >= 3 && (ord & 1u)) {
      verdict = ga ? grouped_key(p, avail, &key) : adfea_key(p, avail, &key);
      kind = kAdfeaKey;
      // the key's entry is its slot token's; a key with no slot token ends
      // the text, and its place is past the last entry
      dest = fpos + feat;
      if (kEmit && dest >= o.nnz) dest = kNone;
      if (kEmit && ga) {  // ... or, in the grouped parse, ends any line: that place is the next line's
        uint32_t e = grouped_field(p, avail, kMaxField);
        if (e > kMaxField) e = grouped_field(p, avail, 0xfffffffeu);
        if (!grouped_follows(p + e, avail - e)) dest = kNone;
      }
    } else if (ord >= 4) {
      if (ga) {  // the slot id of the entry this token completes
        uint32_t id = 0;
        verdict = grouped_slot(p, avail, &id);
        kind = kAdfeaSlot;
        dest = fpos + feat;
        key = id;
      }
      ++feat;
      featm |= 1u << j;
    }
    if (kEmit && kind == kAdfeaSlot && verdict == kFast) {
      if (key < 1 || key >= (uint64_t)kSlotMax)
        atomicMin(&o.words[W_BAD], line);
      else if (dest < o.nnz)
        o.slot[dest] = (uint16_t)key;
    } else if (verdict == kSlow) {
      if (kEmit && spos + slow < o.nslow)  // always, by the counts
        o.slow[spos + slow] = SlowToken{(uint32_t)i, line, dest, (uint32_t)kind};
      ++slow;
    } else if (kEmit && verdict == kReject) {
      atomicMin(&o.words[W_BAD], line);
      if (dest < o.nnz) {
        o.index[dest] = 0;
        o.value[dest] = 0.0;
      }
    } else if (kEmit && kind >= 0) {
      if (kind == kLibsvmLabel || kind == kAdfeaLabel) {
        o.y[dest] = val;
      } else if (dest < o.nnz) {
        o.index[dest] = key;
        if (kind == kLibsvmPair) o.value[dest] = val;
      }
    }
  }
  *nfeat = feat;
  *nslow = slow;
  if (!kEmit || !l.n) return;
  const uint32_t min_tok = libsvm ? 1u : 3u;
  if (l.prev == '\n' && line0 <= rows) o.offset[line0] = fpos;  // a line starts the lane
  for (uint32_t m = nlm; m; m &= m - 1) {
    const uint32_t j = (uint32_t)__ffs((int)m) - 1;
    const uint32_t line = line_at(j);  // the line that ends here
    if (line < rows) {
      o.line_end[line] = (uint32_t)(l.i0 + j);
      if (ord_at(j) + ((stm >> j) & 1u) < min_tok) atomicMin(&o.words[W_BAD], line);
    }
    if (j + 1 < l.n && line + 1 <= rows)  // the next line starts in the lane too
      o.offset[line + 1] = fpos + (uint32_t)__popc(featm & ((2u << j) - 1));
  }
  for (uint32_t m = zero; m; m &= m - 1) {
    const uint32_t line = line_at((uint32_t)__ffs((int)m) - 1);
    if (line < rows) atomicMin(&o.words[W_BAD], line);
  }
  const uint32_t e = l.n - 1;  // a last line without '\n' ends with the text
  if (final && l.i0 + l.n == nbytes && !((nlm >> e) & 1u)) {
    const uint32_t line = line_at(e);
    if (line < rows) {
      o.line_end[line] = (uint32_t)(l.i0 + e);
      if (ord_at(e) + ((stm >> e) & 1u) < min_tok) atomicMin(&o.words[W_BAD], line);
    }
  }
}

__global__ __launch_bounds__(256) void class_kernel(const unsigned char* __restrict__ text,
                                                    uint64_t nbytes, int libsvm, int ga,
                                                    int final, Chunks ch,
                                                    const uint32_t* __restrict__ words,
                                                    uint16_t* __restrict__ lane_cnt) {
  __shared__ uint32_t sh[16];
  const Lane l = load_lane(text, nbytes);
  uint32_t nls, total, after, line, ord;
  lane_counts(l, libsvm, ga, nbytes, &nls, &total, &after);
  lane_state(nls, total, after, ch.line_base[blockIdx.x], ch.ord_base[blockIdx.x], sh, &line, &ord);
  uint32_t feat, slow;
  lane_walk<false>(text, nbytes, libsvm, ga, final, l, line, ord, words[W_ROWS], 0, 0, Emit{},
                   &feat, &slow);
  lane_cnt[(size_t)blockIdx.x * 256u + threadIdx.x] = (uint16_t)(feat | (slow << 8));  // <= 8 each
  uint32_t fsum, ssum;
  (void)block_exscan(feat, sh, &fsum);
  (void)block_exscan(slow, sh + 4, &ssum);
  if (threadIdx.x == 0) {
    ch.feat[blockIdx.x] = fsum;
    ch.slow[blockIdx.x] = ssum;
  }
}

__global__ __launch_bounds__(256) void emit_kernel(const unsigned char* __restrict__ text,
                                                   uint64_t nbytes, int libsvm, int ga,
                                                   int final, Chunks ch,
                                                   const uint16_t* __restrict__ lane_cnt,
                                                   uint32_t rows, Emit o) {
  __shared__ uint32_t sh[16];
  const Lane l = load_lane(text, nbytes);
  uint32_t nls, total, after, line, ord;
  lane_counts(l, libsvm, ga, nbytes, &nls, &total, &after);
  lane_state(nls, total, after, ch.line_base[blockIdx.x], ch.ord_base[blockIdx.x], sh, &line, &ord);
  const uint32_t cnt = lane_cnt[(size_t)blockIdx.x * 256u + threadIdx.x];
  uint32_t tot;
  const uint32_t fpos = ch.feat[blockIdx.x] + block_exscan(cnt & 255u, sh, &tot);
  const uint32_t spos = ch.slow[blockIdx.x] + block_exscan(cnt >> 8, sh + 4, &tot);
  uint32_t feat, slow;
  lane_walk<true>(text, nbytes, libsvm, ga, final, l, line, ord, rows, fpos, spos, o, &feat,
                  &slow);
}

// ---- (6), (7) -------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_kernel(const SlowToken* __restrict__ tok,
                                                    const SlowPatch* __restrict__ patch,
                                                    uint32_t n, Emit o) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const SlowToken t = tok[i];
  const SlowPatch p = patch[i];
  if (!p.ok) {
    atomicMin(&o.words[W_BAD], t.line);
    return;
  }
  if (t.kind == kLibsvmLabel || t.kind == kAdfeaLabel) {
    o.y[t.dest] = p.val;
  } else if (t.kind == kAdfeaSlot) {
    if (t.dest < o.nnz) o.slot[t.dest] = (uint16_t)p.key;
  } else if (t.dest < o.nnz) {
    o.index[t.dest] = p.key;
    if (t.kind == kLibsvmPair) o.value[t.dest] = p.val;
  }
}

// last_idx > idx (example_parser.cc:113): entry j below the one before it,
// unless j is its row's first
__global__ __launch_bounds__(256) void order_kernel(const uint64_t* __restrict__ offset,
                                                    const uint64_t* __restrict__ index,
                                                    uint32_t rows, uint32_t n,
                                                    uint32_t* __restrict__ words) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x + 1;
  if (j >= n || index[j - 1] <= index[j]) return;
  uint32_t lo = 0, hi = rows;  // the last row in [lo, hi) with offset[row] <= j
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (offset[mid] <= j) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  if (offset[lo] != j) atomicMin(&words[W_BAD], lo);
}

__global__ __launch_bounds__(256) void line_kernel(const uint32_t* __restrict__ line_end,
                                                   uint32_t rows, uint32_t* __restrict__ words) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= rows) return;
  const uint64_t start = r ? (uint64_t)line_end[r - 1] + 1 : 0;
  if ((uint64_t)line_end[r] + 1 - start >= kMaxLine - 1) atomicMin(&words[W_BAD], (uint32_t)r);
}

__global__ void verdict_kernel(const uint64_t* __restrict__ offset,
                               const uint32_t* __restrict__ line_end, uint32_t rows,
                               uint32_t* __restrict__ words) {
  if (threadIdx.x || blockIdx.x) return;
  const uint32_t bad = words[W_BAD];
  const uint32_t kept = bad < rows ? bad : rows;
  words[W_ROWS_OUT] = kept;
  words[W_NNZ_OUT] = (uint32_t)offset[kept];
  const uint32_t last = bad < rows ? bad : rows - 1;  // rows > 0 here
  words[W_CONSUMED] = line_end[last];                 // + 1 on the host: it may be 2^32 - 1
}

// OR / AND of the slot ids of the entries kept: the digits the grouping sorts on
__global__ __launch_bounds__(256) void slot_bits_kernel(const uint16_t* __restrict__ slot,
                                                        uint32_t* __restrict__ words) {
  const uint32_t n = words[W_NNZ_OUT];
  uint32_t o = 0, a = 0xffffu;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * 256u) {
    o |= slot[i];
    a &= slot[i];
  }
  for (int s = 32; s >= 1; s >>= 1) {
    o |= __shfl_xor(o, s, 64);
    a &= __shfl_xor(a, s, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicOr(&words[W_SLOT_OR], o);
    atomicAnd(&words[W_SLOT_AND], a);
  }
}

}  // namespace
}  // namespace psg

using psg::fail;

extern "C" {

size_t psg_text_chunk(void) { return psg::kChunk; }

namespace {

int load_text(psg_minibatch* mb, const char* text, size_t nbytes, int format, size_t max_rows,
              int final, bool grouped, psg_text_result* result) {
  using namespace psg;
  if (!mb || !result || (nbytes && !text)) return fail(PSG_ERR_ARG, "null argument");
  if (format != PSG_TEXT_ADFEA && format != PSG_TEXT_LIBSVM)
    return fail(PSG_ERR_ARG, "text format %d", format);
  if (nbytes >= 0xffffffffull) return fail(PSG_ERR_SIZE, "%zu bytes of text >= 2^32 - 1", nbytes);
  const int libsvm = format == PSG_TEXT_LIBSVM;
  const int ga = grouped && !libsvm;  // grouped ADFEA: the line rule changes, slot tokens are read
  const uint32_t want_rows = (uint32_t)std::min<size_t>(max_rows, 0xfffffffeull);
  *result = psg_text_result{0, 0, 0, -1, 0, -1.0};
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;
  mb->state = S_NEW;
  if (!mb->h_text) HIP_TRY(hipHostMalloc((void**)&mb->h_text, 64));
  hipStream_t s = mb->stream;
  const uint32_t nc = blocks_of(nbytes, kChunk);
  uint32_t* h = mb->h_text;
  for (int i = 0; i < W_COUNT; ++i) h[i] = 0;
  h[W_BAD] = kNone;
  h[W_SLOT_AND] = 0xffffu;
  const int tev = 2 * PSG_MB_STAGES;
  const bool timed = mb->prof && mb->tev[tev] && mb->tev[tev + 1];
  if (nc) {
    if (int rc = mb->need_all({{B_TEXT, (size_t)nc * kChunk}, {B_TX_CHUNK, 4 * 7 * (size_t)nc},
                               {B_TX_LANE, 2 * 256 * (size_t)nc}, {B_TX_WORDS, 64}}))
      return rc;
    const unsigned char* d_text = mb->at<unsigned char>(B_TEXT);
    uint32_t* words = mb->at<uint32_t>(B_TX_WORDS);
    const Chunks ch = chunks_of(mb->at<uint32_t>(B_TX_CHUNK), nc);
    HIP_TRY(hipMemcpyAsync(mb->b[B_TEXT].p, text, nbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(words, h, 4 * W_COUNT, hipMemcpyHostToDevice, s));
    if (timed) HIP_TRY(hipEventRecord(mb->tev[tev], s));
    LAUNCH(count_kernel, nc, s, d_text, (uint64_t)nbytes, libsvm, ga, ch);
    LAUNCH(chunk_scan_kernel, 1, s, d_text, (uint64_t)nbytes, nc, ch, want_rows, final, words);
    LAUNCH(class_kernel, nc, s, d_text, (uint64_t)nbytes, libsvm, ga, final, ch, words,
           mb->at<uint16_t>(B_TX_LANE));
    LAUNCH(row_scan_kernel, 2, s, ch.feat, nc, words + W_NNZ);  // W_NNZ, W_SLOW
    if (int rc = launched("text count")) return rc;
    HIP_TRY(hipMemcpyAsync(h, words, 4 * W_COUNT, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // the sizes
  }
  const size_t rows = h[W_ROWS], n = h[W_NNZ], nslow = h[W_SLOW];
  if (int rc = mb_load_begin(mb, rows, n, libsvm != 0)) return rc;
  if (grouped)
    if (int rc = mb->need(B_SLOT, 2 * n)) return rc;
  if (rows) {
    if (int rc = mb->need_all({{B_TX_LINE_END, 4 * rows}, {B_TX_SLOW, sizeof(SlowToken) * nslow},
                               {B_TX_PATCH, sizeof(SlowPatch) * nslow}}))
      return rc;
    const unsigned char* d_text = mb->at<unsigned char>(B_TEXT);
    uint32_t* words = mb->at<uint32_t>(B_TX_WORDS);
    const Chunks ch = chunks_of(mb->at<uint32_t>(B_TX_CHUNK), nc);
    const Emit o{mb->at<uint64_t>(B_OFFSET), mb->at<uint64_t>(B_INDEX), mb->at<double>(B_VALUE),
                 mb->at<double>(B_Y), grouped ? mb->at<uint16_t>(B_SLOT) : nullptr,
                 mb->at<uint32_t>(B_TX_LINE_END), mb->at<SlowToken>(B_TX_SLOW),
                 words, (uint32_t)n, (uint32_t)nslow};
    uint64_t* h_n = (uint64_t*)(h + W_COUNT);  // pinned, and not read into again
    *h_n = n;
    HIP_TRY(hipMemcpyAsync(o.offset + rows, h_n, 8, hipMemcpyHostToDevice, s));
    LAUNCH(emit_kernel, nc, s, d_text, (uint64_t)nbytes, libsvm, ga, final, ch,
           mb->at<uint16_t>(B_TX_LANE), (uint32_t)rows, o);
    if (int rc = launched("text emit")) return rc;
    if (nslow) {
      const size_t need = (sizeof(SlowToken) + sizeof(SlowPatch)) * nslow;
      if (need > mb->h_slow_cap) {
        if (mb->h_slow) HIP_TRY(hipHostFree(mb->h_slow));
        mb->h_slow = nullptr;
        mb->h_slow_cap = 0;
        HIP_TRY(hipHostMalloc(&mb->h_slow, need));
        mb->h_slow_cap = need;
      }
      SlowPatch* h_patch = (SlowPatch*)mb->h_slow;  // 8-byte aligned first
      SlowToken* h_tok = (SlowToken*)(h_patch + nslow);
      HIP_TRY(hipMemcpyAsync(h_tok, o.slow, sizeof(SlowToken) * nslow, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));  // the slow tokens
      resolve_slow((const unsigned char*)text, nbytes, libsvm, grouped, h_tok, nslow, h_patch);
      HIP_TRY(hipMemcpyAsync(mb->b[B_TX_PATCH].p, h_patch, sizeof(SlowPatch) * nslow,
                             hipMemcpyHostToDevice, s));
      LAUNCH(patch_kernel, blocks_of(nslow, 256), s, o.slow, mb->at<SlowPatch>(B_TX_PATCH),
             (uint32_t)nslow, o);
    }
    if (libsvm && n > 1)
      LAUNCH(order_kernel, blocks_of(n - 1, 256), s, o.offset, o.index, (uint32_t)rows,
             (uint32_t)n, words);
    LAUNCH(line_kernel, blocks_of(rows, 256), s, o.line_end, (uint32_t)rows, words);
    hipLaunchKernelGGL(verdict_kernel, dim3(1), dim3(64), 0, s, o.offset, o.line_end,
                       (uint32_t)rows, words);
    if (grouped && n)
      LAUNCH(slot_bits_kernel, std::min<uint32_t>(blocks_of(n, 256), 1024u), s, o.slot, words);
    if (int rc = launched("text verdict")) return rc;
    HIP_TRY(hipMemcpyAsync(h, words, 4 * W_COUNT, hipMemcpyDeviceToHost, s));
  } else {
    HIP_TRY(hipMemsetAsync(mb->b[B_OFFSET].p, 0, 8, s));
  }
  if (timed && nc) HIP_TRY(hipEventRecord(mb->tev[tev + 1], s));
  if (int rc = mb_load_finish(mb, rows, n, libsvm != 0)) return rc;  // waits: h is read
  if (rows) {
    result->rows = h[W_ROWS_OUT];
    result->nnz = h[W_NNZ_OUT];
    result->consumed = (uint64_t)h[W_CONSUMED] + 1;
    if (h[W_BAD] < rows) {
      result->bad_line = h[W_BAD];
      // the rows past the rejected line are dropped: the tail again over the rest
      if (int rc = mb_load_finish(mb, (size_t)result->rows, (size_t)result->nnz, libsvm != 0))
        return rc;
    }
  }
  result->slow_tokens = nslow;
  if (grouped) {
    mb->slot_differ = rows && result->nnz ? (uint64_t)((h[W_SLOT_OR] ^ h[W_SLOT_AND]) & 0xffffu) : 0;
    mb->has_slots = true;
  }
  if (timed && nc) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, mb->tev[tev], mb->tev[tev + 1]));
    result->parse_ms = ms;
  }
  return PSG_OK;
}

}  // namespace

int psg_mb_load_text(psg_minibatch* mb, const char* text, size_t nbytes, int format,
                     size_t max_rows, int final, psg_text_result* result) {
  return load_text(mb, text, nbytes, format, max_rows, final, false, result);
}

int psg_mb_load_text_groups(psg_minibatch* mb, const char* text, size_t nbytes, int format,
                            size_t max_rows, int final, psg_text_result* result) {
  return load_text(mb, text, nbytes, format, max_rows, final, true, result);
}

}  // extern "C"
