// psg_cache.hip -- SlotReader's cache arrays: what
// readOneFile keeps per (file, slot) as .colidx / .rowsiz / .value files of
// snappy streams (src/data/slot_reader.cc:86-141,208-220), and index() /
// offset() / value() (:234-290), which append several files' partitions into
// one resident matrix.
//
// Pack, a loaded minibatch to one cache array, compressed:
//   rowsiz_kernel   offset[r + 1] - offset[r] as uint16; the smallest row of
//                   more than 65535 entries by an integer atomic min
//   narrow_kernel   (float)value, (float)y
//   the array cut into partitions of part_bytes raw bytes, all compressed in
//   one call of the device compressor (psg_snappy_enc.hip); colidx is
//   compressed where it lies, in the index block.
// Load, several files' partitions to one loaded minibatch:
//   every partition of every array of every file in one decoder launch
//   (psg_snappy.hip): colidx into the index block at the file's entry base,
//   rowsiz / value / label into staging where the files lie back to back
//   scan_count / scan_totals / scan_emit   the inclusive scan of the uint16
//                   row sizes into the uint64 offsets, tile totals in 64 bits
//   widen_kernel    (double) of the value and label floats
//   seam_kernel     the offsets at the file seams, read with the partitions'
//                   verdicts in the load's one host wait
// Integer atomics only: the same input gives the same bytes on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/psg.h"
#include "psg_host.h"
#include "psg_internal.h"
#include "psg_minibatch.h"
#include "psg_sort.h"

namespace psg {
namespace {

constexpr uint32_t kScanTile = 2048;  // rows per workgroup of the scan: 8 per lane
constexpr uint32_t kNoRow = 0xffffffffu;
constexpr uint64_t kMaxPart = 0xffffffffull;  // a stream's preamble is a 32-bit varint

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- pack -------------------------------------------------------------------
__global__ __launch_bounds__(256) void rowsiz_kernel(const uint64_t* __restrict__ offset,
                                                     uint32_t rows, uint16_t* __restrict__ out,
                                                     uint32_t* __restrict__ bad) {
  const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (r >= rows) return;
  const uint64_t d = offset[r + 1] - offset[r];
  if (d > 65535ull) atomicMin(bad, (uint32_t)r);
  out[r] = (uint16_t)d;
}

__global__ __launch_bounds__(256) void narrow_kernel(const double* __restrict__ in, uint32_t n,
                                                     float* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}

// ---- load -------------------------------------------------------------------
__global__ __launch_bounds__(256) void widen_kernel(const float* __restrict__ in, uint32_t n,
                                                    double* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

// A lane's 8 consecutive row sizes (0 past the end): one 16-byte load where
// all 8 exist.  siz is 16-byte aligned and i0 a multiple of 8.
__device__ __forceinline__ void load_sizes(const uint16_t* __restrict__ siz, uint64_t i0,
                                           uint32_t rows, uint32_t v[8]) {
  if (i0 + 8 <= rows) {
    const uint4 q = *reinterpret_cast<const uint4*>(siz + i0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    for (uint32_t j = 0; j < 4; ++j) {
      v[2 * j] = w[j] & 0xffffu;
      v[2 * j + 1] = w[j] >> 16;
    }
  } else {
    for (uint32_t j = 0; j < 8; ++j) v[j] = i0 + j < rows ? siz[i0 + j] : 0u;
  }
}

// tile_sum[t] = the sizes of rows [t * kScanTile, (t + 1) * kScanTile)
__global__ __launch_bounds__(256) void scan_count_kernel(const uint16_t* __restrict__ siz,
                                                         uint32_t rows,
                                                         uint64_t* __restrict__ tile_sum) {
  __shared__ uint32_t ws[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 8u;
  uint32_t v[8], c = 0;
  load_sizes(siz, i0, rows, v);
  for (uint32_t j = 0; j < 8; ++j) c += v[j];
  uint32_t tot;  // <= 2048 * 65535: 32 bits hold a tile
  (void)block_exscan(c, ws, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// one workgroup: tile_sum[0 .. nt) becomes its exclusive scan in 64 bits,
// tile_sum[nt] the total
__global__ __launch_bounds__(256) void scan_totals_kernel(uint64_t* __restrict__ tile_sum,
                                                          uint32_t nt) {
  __shared__ uint64_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (uint32_t b = 0; b < nt; b += 256) {
    const uint32_t i = b + threadIdx.x;
    const uint64_t v = i < nt ? tile_sum[i] : 0ull;
    uint64_t inc = v;
    for (uint32_t s = 1; s < 64; s <<= 1) {
      const uint64_t u = __shfl_up((unsigned long long)inc, s, 64);
      if (lane >= s) inc += u;
    }
    __syncthreads();  // the previous round's wsum is read
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t below = 0, tot = 0;
    for (uint32_t k = 0; k < 4; ++k) {
      const uint64_t x = wsum[k];
      if (k < w) below += x;
      tot += x;
    }
    if (i < nt) tile_sum[i] = carry + below + inc - v;
    carry += tot;
  }
  if (threadIdx.x == 0) tile_sum[nt] = carry;
}

// offset[r + 1] = the sizes of rows 0 .. r; offset[0] = 0
__global__ __launch_bounds__(256) void scan_emit_kernel(const uint16_t* __restrict__ siz,
                                                        uint32_t rows,
                                                        const uint64_t* __restrict__ tile_base,
                                                        uint64_t* __restrict__ offset) {
  __shared__ uint32_t ws[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 8u;
  uint32_t v[8], c = 0;
  load_sizes(siz, i0, rows, v);
  for (uint32_t j = 0; j < 8; ++j) c += v[j];
  uint32_t tot;
  uint64_t run = tile_base[blockIdx.x] + block_exscan(c, ws, &tot);
  if (blockIdx.x == 0 && threadIdx.x == 0) offset[0] = 0;
  for (uint32_t j = 0; j < 8; ++j)
    if (i0 + j < rows) {
      run += v[j];
      offset[i0 + j + 1] = run;
    }
}

// out[f] = offset[row_base[f]]: the entries before file f
__global__ __launch_bounds__(256) void seam_kernel(const uint64_t* __restrict__ offset,
                                                   const uint64_t* __restrict__ row_base,
                                                   uint32_t n, uint64_t* __restrict__ out) {
  const uint64_t f = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (f < n) out[f] = offset[row_base[f]];
}

size_t elt_of(int what) {
  switch (what) {
    case PSG_CACHE_COLIDX: return 8;
    case PSG_CACHE_ROWSIZ: return 2;
    default: return 4;
  }
}

const char* name_of(int what) {
  switch (what) {
    case PSG_CACHE_COLIDX: return "colidx";
    case PSG_CACHE_ROWSIZ: return "rowsiz";
    case PSG_CACHE_VALUE: return "value";
    default: return "label";
  }
}

// one stream of the load: where it lies in the caller's file, where it goes
struct Part {
  uint32_t file;
  int32_t what, part;
  uint64_t src, size;  // in the staged bytes
  uint64_t dst, len;   // device address, declared bytes
};

}  // namespace
}  // namespace psg

using psg::fail;

extern "C" {

size_t psg_cache_scan_tile(void) { return psg::kScanTile; }

int psg_cache_pack_bound(size_t raw_bytes, size_t part_bytes, size_t* cap, size_t* nparts) {
  if (!cap || !nparts) return fail(PSG_ERR_ARG, "null argument");
  *cap = *nparts = 0;
  if (part_bytes % 8) return fail(PSG_ERR_ARG, "part_bytes = %zu is no multiple of 8", part_bytes);
  if (raw_bytes == 0) return PSG_OK;
  if (part_bytes == 0 || part_bytes >= raw_bytes) {
    *nparts = 1;
    *cap = psg_snappy_max_compressed_length(raw_bytes);
    return PSG_OK;
  }
  const size_t full = raw_bytes / part_bytes, rest = raw_bytes % part_bytes;
  *nparts = full + (rest ? 1 : 0);
  *cap = full * psg_snappy_max_compressed_length(part_bytes) +
         (rest ? psg_snappy_max_compressed_length(rest) : 0);
  return PSG_OK;
}

int psg_mb_cache_pack(psg_minibatch* mb, int what, size_t part_bytes, void* out, size_t cap,
                      size_t* len, uint64_t* parts, size_t parts_cap, size_t* nparts_out,
                      int64_t* bad_row) {
  using namespace psg;
  if (!mb || !len || !nparts_out || !bad_row) return fail(PSG_ERR_ARG, "null argument");
  *len = *nparts_out = 0;
  *bad_row = -1;
  if (what < PSG_CACHE_COLIDX || what > PSG_CACHE_LABEL)
    return fail(PSG_ERR_ARG, "psg_mb_cache_pack: array %d", what);
  if (mb->state < S_LOADED) return fail(PSG_ERR_ARG, "psg_mb_cache_pack before a load");
  if (what == PSG_CACHE_VALUE && mb->binary)
    return fail(PSG_ERR_ARG, "psg_mb_cache_pack: a binary matrix has no value array");
  const bool per_row = what == PSG_CACHE_ROWSIZ || what == PSG_CACHE_LABEL;
  const size_t n = per_row ? mb->rows : mb->nnz;
  const size_t raw = n * elt_of(what);
  size_t need_cap = 0, np = 0;
  if (int rc = psg_cache_pack_bound(raw, part_bytes, &need_cap, &np)) return rc;
  const size_t pb = np <= 1 ? raw : part_bytes;  // the raw bytes of every partition but the last
  if (pb > kMaxPart) return fail(PSG_ERR_SIZE, "a partition of %zu bytes", pb);
  if (cap < need_cap)
    return fail(PSG_ERR_SIZE, "psg_mb_cache_pack: room for %zu bytes, %zu may be needed", cap,
                need_cap);
  if (parts_cap < np)
    return fail(PSG_ERR_SIZE, "psg_mb_cache_pack: room for %zu partitions of %zu", parts_cap, np);
  if (np == 0) return PSG_OK;  // compressTo of an empty array is an empty array
  if (!out || !parts) return fail(PSG_ERR_ARG, "null output");
  HIP_TRY(hipSetDevice(mb->device));
  if (int rc = mb->settle()) return rc;
  // tables: soff[np + 1] | doff[np] | clen[np] | the bad row
  const size_t tab_bytes = 8 * (3 * np + 2);
  const size_t scr_bytes = snappy_compress_scratch_bytes(raw, np);
  if (int rc = mb->need_all({{B_CA_RAW, what == PSG_CACHE_COLIDX ? 0 : raw},
                             {B_CA_OUT, need_cap},
                             {B_CA_TAB, tab_bytes},
                             {B_CA_SCR, scr_bytes}}))
    return rc;
  std::vector<uint64_t> tab;
  try {
    tab.assign(3 * np + 2, 0);
  } catch (const std::bad_alloc&) {
    return fail(PSG_ERR_OOM, "host allocation");
  }
  uint64_t* h_soff = tab.data();
  uint64_t* h_doff = h_soff + np + 1;
  uint64_t* h_clen = h_doff + np;
  for (size_t i = 0; i < np; ++i) {  // every stream in a slot of the worst case
    h_soff[i] = (uint64_t)i * pb;
    h_doff[i] = (uint64_t)i * psg_snappy_max_compressed_length(pb);
  }
  h_soff[np] = raw;
  h_clen[np] = kNoRow;  // the bad row's word
  hipStream_t s = mb->stream;
  uint64_t* d_tab = mb->at<uint64_t>(B_CA_TAB);
  HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, s));
  uint32_t* d_bad = (uint32_t*)(d_tab + 3 * np + 1);
  const uint8_t* src = mb->at<uint8_t>(B_CA_RAW);
  switch (what) {
    case PSG_CACHE_COLIDX:
      src = mb->at<uint8_t>(B_INDEX);
      break;
    case PSG_CACHE_ROWSIZ:
      LAUNCH(rowsiz_kernel, blocks_of(n, 256), s, mb->at<uint64_t>(B_OFFSET), (uint32_t)n,
             mb->at<uint16_t>(B_CA_RAW), d_bad);
      break;
    default:
      LAUNCH(narrow_kernel, blocks_of(n, 256), s,
             mb->at<double>(what == PSG_CACHE_VALUE ? B_VALUE : B_Y), (uint32_t)n,
             mb->at<float>(B_CA_RAW));
  }
  if (int rc = launched("cache pack")) return rc;
  HIP_TRY(launch_snappy_compress(src, d_tab, np, mb->at<uint8_t>(B_CA_OUT), d_tab + np + 1,
                                 d_tab + 2 * np + 1, mb->b[B_CA_SCR].p, s));
  HIP_TRY(hipMemcpyAsync(h_clen, d_tab + 2 * np + 1, 8 * (np + 1), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // the streams' lengths and the verdict
  const uint32_t bad = (uint32_t)h_clen[np];
  if (bad != kNoRow) {
    *bad_row = bad;
    return fail(PSG_ERR_RANGE, "row %u holds more than 65535 entries", bad);
  }
  for (size_t i = 0; i < np; ++i) {
    const size_t sz = i + 1 < np ? pb : raw - i * pb;
    if (h_clen[i] == 0 || h_clen[i] > psg_snappy_max_compressed_length(sz))
      return fail(PSG_ERR_DEVICE, "cache pack: a stream of %llu bytes for %zu",
                  (unsigned long long)h_clen[i], sz);
  }
  // the worst-case slots as they lie, then the streams moved back to back
  // (every stream moves down: in order, no stream overwrites a later one)
  const size_t span = (size_t)(h_doff[np - 1] + h_clen[np - 1]);
  HIP_TRY(hipMemcpy(out, mb->b[B_CA_OUT].p, span, hipMemcpyDeviceToHost));
  size_t at = 0;
  for (size_t i = 0; i < np; ++i) {
    if (at != h_doff[i]) memmove((char*)out + at, (char*)out + h_doff[i], (size_t)h_clen[i]);
    parts[2 * i] = at;
    parts[2 * i + 1] = h_clen[i];
    at += (size_t)h_clen[i];
  }
  *len = at;
  *nparts_out = np;
  return PSG_OK;
}

int psg_mb_load_cache(psg_minibatch* mb, const psg_cache_file* files, size_t nfiles, int valued,
                      psg_cache_result* result) {
  using namespace psg;
  if (!mb || !result || (nfiles && !files)) return fail(PSG_ERR_ARG, "null argument");
  *result = psg_cache_result{0, 0, -1, -1, -1};
  // whatever happens the previous minibatch is gone
  if (int rc = mb_load_begin(mb, 0, 0, false)) return rc;
  mb->rows = mb->nnz = 0;

  // ---- the host's part: every stream's declared length sizes and places it
  std::vector<Part> pt;
  std::vector<uint64_t> row_base, ent_base;  // [nfiles + 1]
  std::vector<uint8_t> absent;               // the slot is absent from file f
  size_t src_bytes = 0;
  auto bad = [&](int code, size_t f, int what, int64_t part) {
    result->bad_file = (int64_t)f;
    result->bad_what = what;
    result->bad_part = (int32_t)part;
    return code;
  };
  try {
    row_base.assign(nfiles + 1, 0);
    ent_base.assign(nfiles + 1, 0);
    absent.assign(nfiles + 1, 0);
    for (size_t f = 0; f < nfiles; ++f) {
      const psg_cache_array* arr[4] = {&files[f].colidx, &files[f].rowsiz, &files[f].value,
                                       &files[f].label};
      uint64_t count[4] = {0, 0, 0, 0};
      for (int w = 0; w < 4; ++w) {
        if (w == PSG_CACHE_VALUE && !valued) continue;
        const psg_cache_array& a = *arr[w];
        if (a.nbytes == 0) continue;  // assemblePartitions of an empty file: an empty array
        if (!a.data || (a.nparts && !a.parts))
          return bad(fail(PSG_ERR_ARG, "file %zu: null %s", f, name_of(w)), f, w, -1);
        const uint64_t whole[2] = {0, a.nbytes};
        const size_t np = a.nparts ? a.nparts : 1;
        const uint64_t* pr = a.nparts ? a.parts : whole;
        const size_t base = src_bytes;
        src_bytes = align_up(src_bytes + a.nbytes, 16);
        uint64_t bytes = 0;
        for (size_t p = 0; p < np; ++p) {
          const uint64_t start = pr[2 * p], size = pr[2 * p + 1];
          if (start > a.nbytes || size > a.nbytes - start)  // CHECK_LE(first + second, memSize())
            return bad(fail(PSG_ERR_SIZE, "file %zu: %s partition %zu is [%llu, +%llu) of %zu bytes",
                            f, name_of(w), p, (unsigned long long)start, (unsigned long long)size,
                            a.nbytes),
                       f, w, (int64_t)p);
          if (size == 0) continue;  // uncompressFrom of 0 bytes: nothing
          size_t dl = 0;
          if (size >= (1ull << 31) ||
              psg_snappy_uncompressed_length((const char*)a.data + start, size, &dl) != PSG_OK)
            return bad(fail(PSG_ERR_ARG, "file %zu: %s partition %zu is no snappy stream", f,
                            name_of(w), p),
                       f, w, (int64_t)p);
          if (dl % elt_of(w))
            return bad(fail(PSG_ERR_SIZE, "file %zu: %s partition %zu holds %zu bytes", f,
                            name_of(w), p, dl),
                       f, w, (int64_t)p);
          // dst: for now the offset in the file's array
          pt.push_back(Part{(uint32_t)f, w, (int32_t)p, base + start, size, bytes, dl});
          bytes += dl;
        }
        count[w] = bytes / elt_of(w);
      }
      const uint64_t ex = files[f].num_ex;
      // a slot absent from this file: num_ex empty rows
      absent[f] = count[PSG_CACHE_COLIDX] == 0 && count[PSG_CACHE_ROWSIZ] == 0 &&
                  count[PSG_CACHE_VALUE] == 0;
      if (!absent[f] && count[PSG_CACHE_ROWSIZ] != ex)
        return bad(fail(PSG_ERR_SIZE, "file %zu: %llu row sizes, num_ex = %llu", f,
                        (unsigned long long)count[PSG_CACHE_ROWSIZ], (unsigned long long)ex),
                   f, PSG_CACHE_ROWSIZ, -1);
      if (count[PSG_CACHE_LABEL] != ex)
        return bad(fail(PSG_ERR_SIZE, "file %zu: %llu labels, num_ex = %llu", f,
                        (unsigned long long)count[PSG_CACHE_LABEL], (unsigned long long)ex),
                   f, PSG_CACHE_LABEL, -1);
      if (valued && count[PSG_CACHE_VALUE] != count[PSG_CACHE_COLIDX])
        return bad(fail(PSG_ERR_SIZE, "file %zu: %llu values of %llu entries", f,
                        (unsigned long long)count[PSG_CACHE_VALUE],
                        (unsigned long long)count[PSG_CACHE_COLIDX]),
                   f, PSG_CACHE_VALUE, -1);
      row_base[f + 1] = row_base[f] + ex;
      ent_base[f + 1] = ent_base[f] + count[PSG_CACHE_COLIDX];
      if (row_base[f + 1] >= 0xffffffffull)
        return bad(fail(PSG_ERR_SIZE, "%llu rows >= 2^32 - 1",
                        (unsigned long long)row_base[f + 1]), f, -1, -1);
      if (ent_base[f + 1] >= 0xffffffffull)  // psg_mb_load's limit
        return bad(fail(PSG_ERR_SIZE, "%llu entries >= 2^32 - 1: positions are uint32",
                        (unsigned long long)ent_base[f + 1]), f, -1, -1);
    }
  } catch (const std::bad_alloc&) {
    return fail(PSG_ERR_OOM, "host allocation");
  }
  const size_t rows = (size_t)row_base[nfiles], n = (size_t)ent_base[nfiles];
  const size_t np = pt.size();
  const bool val = valued != 0;

  // ---- blocks.  staging: rowsiz[rows] | value[n] | label[rows]
  const size_t o_val = align_up(2 * rows, 256), o_lab = o_val + align_up(val ? 4 * n : 0, 256);
  const size_t out_bytes = o_lab + 4 * rows;
  const uint32_t nt = blocks_of(rows, kScanTile);
  // tables: (begin, end)[np] | dst[np] | len[np] | row_base[nfiles + 1] |
  // seams[nfiles + 1] | tile sums[nt + 1] | status[np]
  const size_t o_dst = 2 * np, o_len = o_dst + np, o_rb = o_len + np, o_seam = o_rb + nfiles + 1;
  const size_t o_tile = o_seam + nfiles + 1, o_stat = o_tile + nt + 1;
  const size_t tab_words = o_stat + (np + 1) / 2;
  if (int rc = mb_load_begin(mb, rows, n, val)) return rc;
  if (int rc = mb->need_all({{B_CA_RAW, src_bytes},
                             {B_CA_OUT, out_bytes},
                             {B_CA_TAB, 8 * tab_words},
                             {B_CA_SCR, np ? snappy_scratch_bytes(np) : 0}}))
    return rc;
  std::vector<uint64_t> tab;
  std::vector<int32_t> h_stat;
  std::vector<uint64_t> h_seam;
  try {
    tab.assign(o_tile, 0);
    h_stat.assign(np, 0);
    h_seam.assign(nfiles + 1, 0);
  } catch (const std::bad_alloc&) {
    return fail(PSG_ERR_OOM, "host allocation");
  }
  hipStream_t s = mb->stream;
  uint8_t* d_src = mb->at<uint8_t>(B_CA_RAW);
  uint8_t* d_out = mb->at<uint8_t>(B_CA_OUT);
  uint64_t* d_tab = mb->at<uint64_t>(B_CA_TAB);
  for (size_t i = 0; i < np; ++i) {
    const Part& p = pt[i];
    tab[2 * i] = (uint64_t)(d_src + p.src);
    tab[2 * i + 1] = tab[2 * i] + p.size;
    uint64_t to;
    switch (p.what) {
      case PSG_CACHE_COLIDX: to = (uint64_t)mb->b[B_INDEX].p + 8 * ent_base[p.file]; break;
      case PSG_CACHE_ROWSIZ: to = (uint64_t)d_out + 2 * row_base[p.file]; break;
      case PSG_CACHE_VALUE: to = (uint64_t)d_out + o_val + 4 * ent_base[p.file]; break;
      default: to = (uint64_t)d_out + o_lab + 4 * row_base[p.file];
    }
    tab[o_dst + i] = to + p.dst;
    tab[o_len + i] = p.len;
  }
  for (size_t f = 0; f <= nfiles; ++f) tab[o_rb + f] = row_base[f];
  HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), 8 * o_tile, hipMemcpyHostToDevice, s));
  // the files' bytes, each array as it lies
  {
    size_t at = 0;
    for (size_t f = 0; f < nfiles; ++f) {
      const psg_cache_array* arr[4] = {&files[f].colidx, &files[f].rowsiz, &files[f].value,
                                       &files[f].label};
      for (int w = 0; w < 4; ++w) {
        if ((w == PSG_CACHE_VALUE && !val) || arr[w]->nbytes == 0) continue;
        HIP_TRY(hipMemcpyAsync(d_src + at, arr[w]->data, arr[w]->nbytes, hipMemcpyHostToDevice, s));
        at = align_up(at + arr[w]->nbytes, 16);
      }
      if (absent[f] && files[f].num_ex)
        HIP_TRY(hipMemsetAsync(d_out + 2 * row_base[f], 0, 2 * (size_t)files[f].num_ex, s));
    }
  }
  int32_t* d_stat = (int32_t*)(d_tab + o_stat);
  if (np) {
    // every partition in one launch: part i from its (begin, end) to the
    // device address dst[i], which must be len[i] bytes
    HIP_TRY(launch_snappy(nullptr, d_tab, np, nullptr, d_tab + o_dst, d_tab + o_len, d_stat,
                          mb->b[B_CA_SCR].p, s, nullptr, true));
    HIP_TRY(hipMemcpyAsync(h_stat.data(), d_stat, 4 * np, hipMemcpyDeviceToHost, s));
  }
  uint64_t* offset = mb->at<uint64_t>(B_OFFSET);
  if (rows) {
    const uint16_t* siz = (const uint16_t*)d_out;
    LAUNCH(scan_count_kernel, nt, s, siz, (uint32_t)rows, d_tab + o_tile);
    LAUNCH(scan_totals_kernel, 1, s, d_tab + o_tile, nt);
    LAUNCH(scan_emit_kernel, nt, s, siz, (uint32_t)rows, d_tab + o_tile, offset);
    LAUNCH(widen_kernel, blocks_of(rows, 256), s, (const float*)(d_out + o_lab), (uint32_t)rows,
           mb->at<double>(B_Y));
  } else {
    HIP_TRY(hipMemsetAsync(offset, 0, 8, s));
  }
  if (val && n)
    LAUNCH(widen_kernel, blocks_of(n, 256), s, (const float*)(d_out + o_val), (uint32_t)n,
           mb->at<double>(B_VALUE));
  LAUNCH(seam_kernel, blocks_of(nfiles + 1, 256), s, offset, d_tab + o_rb, (uint32_t)(nfiles + 1),
         d_tab + o_seam);
  if (int rc = launched("cache load")) return rc;
  HIP_TRY(hipMemcpyAsync(h_seam.data(), d_tab + o_seam, 8 * (nfiles + 1), hipMemcpyDeviceToHost, s));
  // row_of's search and the keys' OR / AND stay in their blocks whatever the
  // offsets and ids hold, so the verdicts can wait for the load's own wait
  if (int rc = mb_load_finish(mb, rows, n, val)) return rc;
  auto drop = [&]() {
    mb->state = S_NEW;
    mb->rows = mb->nnz = 0;
  };
  for (size_t i = 0; i < np; ++i)
    if (h_stat[i] != 0) {
      drop();
      const Part& p = pt[i];
      return bad(fail(PSG_ERR_ARG, "file %u: %s partition %d is a corrupt snappy stream", p.file,
                      name_of(p.what), p.part),
                 p.file, p.what, p.part);
    }
  for (size_t f = 0; f < nfiles; ++f)
    if (h_seam[f + 1] - h_seam[f] != ent_base[f + 1] - ent_base[f]) {
      drop();
      return bad(fail(PSG_ERR_SIZE, "file %zu: the row sizes sum to %llu, %llu entries", f,
                      (unsigned long long)(h_seam[f + 1] - h_seam[f]),
                      (unsigned long long)(ent_base[f + 1] - ent_base[f])),
                 f, PSG_CACHE_ROWSIZ, -1);
    }
  result->rows = rows;
  result->nnz = n;
  return PSG_OK;
}

}  // extern "C"
