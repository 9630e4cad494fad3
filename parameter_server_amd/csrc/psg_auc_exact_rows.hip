// psg_auc_exact_rows.hip -- the exact rank AUC (Evaluation<double>::auc,
// src/base/evaluation.h:17-44) of every column of a row-major prediction
// matrix predict[n][m] against one label array: psg_auc_exact_rows_dev of
// include/psg.h.  Column j is bit for bit psg_auc_exact of that column alone.
//
// A 64-bit prediction key leaves no room for a model id, and needs none: every
// model has n predictions, so model j owns [j * n, (j + 1) * n) of every array
// and the id of an element is where it lies.
//
// (1) xr_keys_kernel: a tile of kRowsTile rows x m predictions is read as one
//     linear run, every prediction becomes exact_keys_kernel's key, the tile
//     is transposed through LDS and leaves as m column segments; NaNs are
//     counted per model and the OR / AND of all keys folded for the host.
// (2) A stable 8-bit LSD radix sort of all m segments at once, the row as
//     payload: per pass one count launch, one scan launch and one scatter
//     launch whose tiles never straddle a segment.  psg_sort.h's per-lane
//     keys, its wave ranking (match_digit) and its row_scan_kernel are used
//     as they are; the segmented count and scatter are this file's.
// (3) The area: the positives sorted before each element of its segment
//     (count, scan per segment, emit), summed over the negatives in uint64,
//     one atomic per wave.  The "positive" flag y[row] > 0 is gathered once,
//     by the count, and kept as one byte per lane for the emit.
// Kernels first, the entry points after them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/psg.h"
#include "psg_auc_dev.h"
#include "psg_host.h"
#include "psg_sort.h"

namespace psg {
namespace {

constexpr uint32_t kRowsTile = 128;  // rows per transpose tile; divides 256
constexpr uint32_t kMaxM = PSG_FTRL_MAX_MODELS;
static_assert(256 % kRowsTile == 0 && kRowsTile % 32 == 0 && kMaxM == 32,
              "xr_keys_kernel: lanes per column, pad period, bad[]");

// The LDS word (8 bytes; a b64 access serves 32 lanes a cycle from 32 such
// words) of row r, column j of a tile.  Rows are m words apart, and after
// every 32 / g rows, g = gcd(m, 32), one more word is skipped:
//  - the column side reads 32 consecutive rows of one column: r * m alone
//    takes 32 / g residues mod 32, each a multiple of g, g times over; the
//    skip tells the g repeats apart, so the 32 words differ mod 32;
//  - the row side writes 32 consecutive elements e = r * m + j, e a multiple
//    of 32 at the first: the skip changes where e is a multiple of 32 m / g,
//    never inside such a group, so the 32 words are consecutive.
__device__ __forceinline__ uint32_t tile_word(uint32_t r, uint32_t j, uint32_t m, uint32_t g) {
  return r * m + j + ((r * g) >> 5);
}
inline uint32_t gcd32(uint32_t m) { return m & (0u - m); }  // 1 <= m <= 32
inline size_t tile_bytes(uint32_t m) {
  return 8 * ((size_t)kRowsTile * m + ((kRowsTile * gcd32(m)) >> 5));
}

// ---- (1) --------------------------------------------------------------------
// key[j * n + i] = the key of predict[i * m + j]; nan[j] += model j's NaNs;
// orand[0] |= every key, orand[1] &= every key
__global__ __launch_bounds__(256) void xr_keys_kernel(const double* __restrict__ predict,
                                                      uint32_t n, uint32_t m, uint32_t g,
                                                      uint32_t ntile, uint64_t* __restrict__ key,
                                                      unsigned long long* __restrict__ orand,
                                                      unsigned long long* __restrict__ nan) {
  extern __shared__ uint64_t tile[];  // tile_bytes(m)
  __shared__ uint32_t bad[kMaxM];
  __shared__ uint64_t fold[2][4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  if (tid < kMaxM) bad[tid] = 0;
  uint64_t o = 0, a = ~0ull;
  for (uint32_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const uint32_t r0 = t * kRowsTile;
    const uint32_t rows = n - r0 < kRowsTile ? n - r0 : kRowsTile;
    const uint32_t cnt = rows * m;
    const double* src = predict + (uint64_t)r0 * m;
    __syncthreads();  // the tile before this one is read out (and bad[] is zero)
    for (uint32_t e = tid; e < cnt; e += 256u) {
      const double p = src[e];
      const uint32_t r = e / m, j = e - r * m;
      if (p != p) atomicAdd(&bad[j], 1u);
      const uint64_t b = p == 0 ? 0ull : (uint64_t)__double_as_longlong(p);
      const uint64_t k = (b & kSignBit) ? ~b : b | kSignBit;
      tile[tile_word(r, j, m, g)] = k;
      o |= k;
      a &= k;
    }
    __syncthreads();
    const uint32_t r = tid & (kRowsTile - 1);
    if (r < rows)
      for (uint32_t j = tid / kRowsTile; j < m; j += 256u / kRowsTile)
        key[(uint64_t)j * n + r0 + r] = tile[tile_word(r, j, m, g)];
  }
  for (int s = 32; s >= 1; s >>= 1) {
    o |= __shfl_xor(o, s, 64);
    a &= __shfl_xor(a, s, 64);
  }
  if (lane == 0) {
    fold[0][w] = o;
    fold[1][w] = a;
  }
  __syncthreads();
  if (tid == 0) {
    atomicOr(orand, (unsigned long long)(fold[0][0] | fold[0][1] | fold[0][2] | fold[0][3]));
    atomicAnd(orand + 1, (unsigned long long)(fold[1][0] & fold[1][1] & fold[1][2] & fold[1][3]));
  }
  if (tid < m && bad[tid]) atomicAdd(&nan[tid], (unsigned long long)bad[tid]);
}

// ---- (2) --------------------------------------------------------------------
// Tile t of the grid is tile t % tps of segment t / tps, tps = tiles of one
// segment; the segment's keys start at seg * n.
// counts[(seg * 256 + d) * tps + tl] = pairs of that tile whose digit is d
__global__ __launch_bounds__(256) void xr_count_kernel(const uint64_t* __restrict__ keys,
                                                       uint32_t n, uint32_t tps, int shift,
                                                       uint32_t* __restrict__ counts) {
  __shared__ uint32_t h[256];
  const uint32_t t = xcd_index(blockIdx.x, gridDim.x);
  const uint32_t seg = t / tps, tl = t - seg * tps;
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t* k = keys + (uint64_t)seg * n;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)tl * kSortTile + (uint64_t)w * kWaveSpan + lane;
#pragma unroll 4
  for (int j = 0; j < kSortKPT; ++j) {
    const uint64_t i = base + (uint64_t)j * 64u;
    const bool valid = i < n;
    const uint32_t d = valid ? (uint32_t)(k[i] >> shift) & 255u : 0u;
    const uint64_t mt = match_digit(d, valid);
    if (valid && (mt & ((1ull << lane) - 1)) == 0)  // first lane of its group
      atomicAdd(&h[d], (uint32_t)__popcll(mt));
  }
  __syncthreads();
  counts[((size_t)seg * 256u + threadIdx.x) * tps + tl] = h[threadIdx.x];
}

// pin null: the payload is the place in the segment, i.e. the row (the first
// pass); kout null: the keys are not needed again (the last pass).
// counts: scanned along each (segment, digit) row; dtotal[seg * 256 + d]
__global__ __launch_bounds__(256) void xr_scatter_kernel(
    const uint64_t* __restrict__ kin, const uint32_t* __restrict__ pin, uint64_t* __restrict__ kout,
    uint32_t* __restrict__ pout, uint32_t n, uint32_t tps, int shift,
    const uint32_t* __restrict__ counts, const uint32_t* __restrict__ dtotal) {
  __shared__ uint32_t cnt[4][256];
  __shared__ uint32_t dbase[256];
  __shared__ uint32_t ws[4];
  const uint32_t t = xcd_index(blockIdx.x, gridDim.x);
  const uint32_t seg = t / tps, tl = t - seg * tps;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const uint64_t sbase = (uint64_t)seg * n;
  for (int i = 0; i < 4; ++i) cnt[i][tid] = 0;
  {  // first index within the segment of digit `tid` for this tile
    uint32_t tot;
    const uint32_t ex = block_exscan(dtotal[seg * 256u + tid], ws, &tot);
    dbase[tid] = ex + counts[((size_t)seg * 256u + tid) * tps + tl];
  }
  __syncthreads();
  // as sort_scatter_kernel: the wave's counters, read by every lane and then
  // advanced by the last lane of each group, in the wave's own order
  volatile uint32_t* mine = cnt[w];
  const uint64_t base = (uint64_t)tl * kSortTile + (uint64_t)w * kWaveSpan + lane;
  uint64_t key[kSortKPT];
  uint32_t off[kSortKPT];
#pragma unroll
  for (int j = 0; j < kSortKPT; ++j) {
    const uint64_t i = base + (uint64_t)j * 64u;
    const bool valid = i < n;
    key[j] = valid ? kin[sbase + i] : 0;
    const uint32_t d = (uint32_t)(key[j] >> shift) & 255u;
    const uint64_t mt = match_digit(d, valid);
    const uint32_t before = mine[d];
    const uint32_t below = (uint32_t)__popcll(mt & ((1ull << lane) - 1));
    const uint32_t group = (uint32_t)__popcll(mt);
    __builtin_amdgcn_wave_barrier();
    if (valid && below + 1 == group) mine[d] = before + group;
    __builtin_amdgcn_wave_barrier();
    off[j] = before + below;
  }
  __syncthreads();
  {  // the waves' totals of digit `tid` become their exclusive prefix
    uint32_t run = 0;
    for (int i = 0; i < 4; ++i) {
      const uint32_t x = cnt[i][tid];
      cnt[i][tid] = run;
      run += x;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSortKPT; ++j) {
    const uint64_t i = base + (uint64_t)j * 64u;
    if (i < n) {
      const uint32_t d = (uint32_t)(key[j] >> shift) & 255u;
      const uint32_t dst = dbase[d] + cnt[w][d] + off[j];
      if (dst < n) {  // always, by the counts; keeps a bad count in its segment
        if (kout) kout[sbase + dst] = key[j];
        pout[sbase + dst] = pin ? pin[sbase + i] : (uint32_t)i;
      }
    }
  }
}

// no digit differs in any segment: every segment is sorted as it stands
__global__ __launch_bounds__(256) void xr_identity_kernel(uint32_t* __restrict__ pout, uint32_t n,
                                                          uint64_t total) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * 256u)
    pout[i] = (uint32_t)(i % n);
}

// ---- (3) --------------------------------------------------------------------
// Workgroup b: flag tile b % ftps of segment b / ftps; a lane owns 8
// consecutive sorted elements, as in psg_sort.h's flag scans.
// fbits[b * 256 + lane]: bit k = element k of the lane is a positive
// (evaluation.h:36); tile_sum[b] = the tile's positives
__global__ __launch_bounds__(256) void xr_flag_count_kernel(const uint32_t* __restrict__ spos,
                                                            const double* __restrict__ y,
                                                            uint32_t n, uint32_t ftps,
                                                            uint8_t* __restrict__ fbits,
                                                            uint32_t* __restrict__ tile_sum) {
  __shared__ uint32_t ws[4];
  const uint32_t seg = blockIdx.x / ftps, tl = blockIdx.x - seg * ftps;
  const uint32_t* sp = spos + (uint64_t)seg * n;
  const uint64_t i0 = (uint64_t)tl * kFlagTile + threadIdx.x * 8u;
  uint32_t bits = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k)
    if (i0 + k < n) {
      const uint32_t at = sp[i0 + k];
      if (at < n && y[at] > 0) bits |= 1u << k;  // at < n always, by the sort
    }
  fbits[(size_t)blockIdx.x * 256u + threadIdx.x] = (uint8_t)bits;
  uint32_t tot;
  (void)block_exscan((uint32_t)__popc(bits), ws, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// tile_base: tile_sum scanned along each segment.  area[seg] += over the
// segment's negatives, the positives sorted before them.
__global__ __launch_bounds__(256) void xr_area_kernel(const uint8_t* __restrict__ fbits,
                                                      const uint32_t* __restrict__ tile_base,
                                                      uint32_t n, uint32_t ftps,
                                                      unsigned long long* __restrict__ area) {
  __shared__ uint32_t ws[4];
  const uint32_t seg = blockIdx.x / ftps, tl = blockIdx.x - seg * ftps;
  const uint64_t i0 = (uint64_t)tl * kFlagTile + threadIdx.x * 8u;
  const uint32_t bits = fbits[(size_t)blockIdx.x * 256u + threadIdx.x];
  uint32_t tot;
  uint32_t ex = tile_base[blockIdx.x] + block_exscan((uint32_t)__popc(bits), ws, &tot);
  uint64_t a = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k)
    if (i0 + k < n) {
      const bool positive = (bits >> k) & 1u;
      a += positive ? 0u : ex;
      ex += positive ? 1u : 0u;
    }
  for (int s = 32; s >= 1; s >>= 1) a += __shfl_xor(a, s, 64);
  if ((threadIdx.x & 63u) == 0 && a) atomicAdd(&area[seg], (unsigned long long)a);
}

}  // namespace
}  // namespace psg

// ------------------------------------------------------------------- host --
using namespace psg;

namespace {

constexpr size_t kMaxItems = 0xffffffffull;  // places and ranks are uint32

// the device words (8 bytes each): the OR and the AND of the keys, nan[32],
// area[32], then as u32 the positives of each segment [32]; the digit totals
// [m * 256] u32 follow
constexpr size_t kOrAnd = 0, kNan = 2, kArea = kNan + kMaxM, kPos = kArea + kMaxM,
                 kWords = kPos + kMaxM / 2;

int check_args(int m, size_t n) {
  if (m < 1 || m > (int)kMaxM)
    return fail(PSG_ERR_ARG, "psg_auc_exact_rows: m = %d outside 1 .. %u", m, kMaxM);
  if (n >= kMaxItems || n * (size_t)m >= kMaxItems)
    return fail(PSG_ERR_SIZE, "%zu examples of %d models >= 2^32 - 1 predictions", n, m);
  return PSG_OK;
}

}  // namespace

extern "C" {

size_t psg_auc_exact_rows_tile(void) { return kRowsTile; }

int psg_auc_exact_rows_dev(psg_ctx* ctx, const double* y_dev, const double* predict_dev, size_t n_z,
                           int m_i, double* auc, void* stream) {
  if (!ctx || !auc || (n_z && (!y_dev || !predict_dev))) return fail(PSG_ERR_ARG, "null argument");
  if (int rc = check_args(m_i, n_z)) return rc;
  const uint32_t m = (uint32_t)m_i;
  const double zero = 0.0;
  if (n_z == 0) {
    for (uint32_t j = 0; j < m; ++j) auc[j] = zero / zero;  // area /= 0 * 0, evaluation.h:42
    return PSG_OK;
  }
  int device, dtype;
  hipStream_t cs;
  ctx_info(ctx, &device, &dtype, &cs);
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = stream ? (hipStream_t)stream : cs;
  const uint32_t n = (uint32_t)n_z;
  const size_t total = n_z * m;
  const uint32_t tps = blocks_of(n, kSortTile), ftps = blocks_of(n, kFlagTile);
  const uint32_t ntiles = m * tps, nft = m * ftps;
  // one block: the words and digit totals, then every array (each a multiple of 8 bytes)
  const size_t small = 8 * kWords + 4 * 256 * (size_t)m;
  const size_t r8 = (4 * total + 7) / 8 * 8;
  const size_t sizes[] = {small, 8 * total, 8 * total, r8, r8, 4 * 256 * (size_t)ntiles,
                          (4 * (size_t)nft + 7) / 8 * 8, 256 * (size_t)nft};
  size_t off[9] = {0};
  for (int i = 0; i < 8; ++i) off[i + 1] = off[i] + sizes[i];
  char* base = nullptr;
  HIP_TRY(hipMalloc((void**)&base, off[8]));
  unsigned long long h_small[kWords] = {0};
  h_small[kOrAnd + 1] = ~0ull;
  int rc = [&]() -> int {
    unsigned long long* d_small = (unsigned long long*)base;
    uint32_t* dtotal = (uint32_t*)(d_small + kWords);
    uint64_t* key_a = (uint64_t*)(base + off[1]);
    uint64_t* key_b = (uint64_t*)(base + off[2]);
    uint32_t* pos_a = (uint32_t*)(base + off[3]);
    uint32_t* pos_b = (uint32_t*)(base + off[4]);
    uint32_t* counts = (uint32_t*)(base + off[5]);
    uint32_t* ts = (uint32_t*)(base + off[6]);
    uint8_t* fbits = (uint8_t*)(base + off[7]);
    HIP_TRY(hipMemcpyAsync(d_small, h_small, sizeof h_small, hipMemcpyHostToDevice, s));
    // (1)
    const uint32_t nrt = blocks_of(n, kRowsTile);
    hipLaunchKernelGGL(xr_keys_kernel, dim3(std::min(nrt, kGridCap)), dim3(256), tile_bytes(m), s,
                       predict_dev, n, m, gcd32(m), nrt, key_b, d_small + kOrAnd, d_small + kNan);
    if (int e = launched("exact auc rows keys")) return e;
    HIP_TRY(hipMemcpyAsync(h_small, d_small, 8 * kArea, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t j = 0; j < m; ++j)
      if (h_small[kNan + j])  // the comparator is no strict weak order then
        return fail(PSG_ERR_ARG, "psg_auc_exact_rows: column %u has %llu NaN predictions", j,
                    h_small[kNan + j]);
    // (2) the digits that differ somewhere, in any segment
    const uint64_t differ = h_small[kOrAnd] ^ h_small[kOrAnd + 1];
    int last = -1;
    for (int d = 0; d < 8; ++d)
      if ((differ >> (8 * d)) & 255u) last = d;
    const uint64_t* kin = key_b;
    const uint32_t* pin = nullptr;
    uint64_t* kout = key_a;
    uint32_t* pout = pos_a;
    for (int d = 0; d <= last; ++d) {
      if (((differ >> (8 * d)) & 255u) == 0) continue;  // the same digit in every key
      LAUNCH(xr_count_kernel, ntiles, s, kin, n, tps, 8 * d, counts);
      LAUNCH(row_scan_kernel, 256 * m, s, counts, tps, dtotal);
      LAUNCH(xr_scatter_kernel, ntiles, s, kin, pin, d == last ? nullptr : kout, pout, n, tps,
             8 * d, counts, dtotal);
      kin = kout;
      pin = pout;
      const bool to_b = kout == key_a;
      kout = to_b ? key_b : key_a;
      pout = to_b ? pos_b : pos_a;
    }
    if (last < 0) {
      LAUNCH(xr_identity_kernel, std::min(blocks_of(total, 256), kGridCap), s, pout, n,
             (uint64_t)total);
      pin = pout;
    }
    if (int e = launched("exact auc rows sort")) return e;
    // (3)
    LAUNCH(xr_flag_count_kernel, nft, s, pin, y_dev, n, ftps, fbits, ts);
    LAUNCH(row_scan_kernel, m, s, ts, ftps, (uint32_t*)(d_small + kPos));
    LAUNCH(xr_area_kernel, nft, s, fbits, ts, n, ftps, d_small + kArea);
    if (int e = launched("exact auc rows area")) return e;
    HIP_TRY(hipMemcpyAsync(h_small + kArea, d_small + kArea, 8 * (kWords - kArea),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return PSG_OK;
  }();
  if (rc != PSG_OK) (void)hipStreamSynchronize(s);
  (void)hipFree(base);
  if (rc != PSG_OK) return rc;
  // the positives are the labels', the same in every segment: segment 0's
  const uint64_t pos = h_small[kPos] & 0xffffffffull;
  if (pos > n_z) return fail(PSG_ERR_DEVICE, "%llu positives of %zu examples",
                             (unsigned long long)pos, n_z);
  for (uint32_t j = 0; j < m; ++j) {
    double area = (double)h_small[kArea + j];
    area /= (double)pos * (double)(n_z - pos);  // evaluation.h:42
    auc[j] = area < 0.5 ? 1 - area : area;
  }
  return PSG_OK;
}

int psg_auc_exact_rows(psg_ctx* ctx, const double* y, const double* predict, size_t n, int m,
                       double* auc) {
  if (!ctx || !auc || (n && (!y || !predict))) return fail(PSG_ERR_ARG, "null argument");
  if (int rc = check_args(m, n)) return rc;
  if (n == 0) return psg_auc_exact_rows_dev(ctx, nullptr, nullptr, 0, m, auc, nullptr);
  int device, dtype;
  hipStream_t cs;
  ctx_info(ctx, &device, &dtype, &cs);
  HIP_TRY(hipSetDevice(device));
  const size_t total = n * (size_t)m;
  double* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 8 * (n + total)));
  int rc = PSG_OK;
  if (hipMemcpy(d, y, 8 * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d + n, predict, 8 * total, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    rc = fail(PSG_ERR_DEVICE, "psg_auc_exact_rows: copy to the device");
  }
  if (rc == PSG_OK) rc = psg_auc_exact_rows_dev(ctx, d, d + n, n, m, auc, nullptr);
  (void)hipFree(d);
  return rc;
}

}  // extern "C"
