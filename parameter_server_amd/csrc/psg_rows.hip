// psg_rows.hip -- row-valued pushes: every key carries a row of k values,
// the k values of a key next to each other (the layout sliceKeyOrderedMsg
// cuts at lr * (val.size() / key.size()), system/message.h:116).  The fold of
// such pushes into the server's rows, the pull reply for rows, and the plan
// API behind them (include/psg.h, "Row-valued pushes").
//
// Semantics: the scalar fold (psg_tile.hip; KVVector::serialSetValue /
// parallelSetValue, kv_vector.h:84-204) applied to every column: the first
// non-empty push assigns its rows, every other push adds element by element
// in arrival order (onto +0.0 where no push held the key before), and the
// serial path's "+0.0 for absent pushes" is ONE
// trailing +0.0 on every element of a row some non-empty push lacked.
//
// Shape:
//   * rows_cuts_kernel: one wave per (push, tile boundary) does the
//     lower_bound of the tile's first server key in the push (wave_search),
//     so push p's keys of tile t are S_p[cut(p, t), cut(p, t + 1)).  Tiles
//     follow D by slot count; nothing is kept from run to run.
//   * rows_fold_kernel: one workgroup per tile of T slots, T from k and the
//     value type (psg_rows.h) so that acc[T][k] stays within 64 KB of LDS and
//     two workgroups share a CU.  A row belongs to a group of L lanes, each
//     moving E elements per access (16 B when the row bytes and every base
//     pointer allow it, element by element otherwise).  Pushes are folded in
//     arrival order with one LDS barrier per push that has keys in the tile:
//     keys are unique within a push, so all four waves work on one push's
//     rows at once and touch distinct slots; a group holds kItemRows rows per
//     step and the next step's rows and keys (of the same or the next push)
//     are in flight while this step's keys are searched in LDS and its rows
//     folded, since a row's address depends on its index in the push only.
//     One contributor count per slot (not per element) decides assign or
//     add, the trailing +0.0 and the zero rows.
//   * rows_gather_kernel: 256 requests per workgroup, searched one per lane
//     inside the span two wave searches bound (as psg_kernels.hip's gather),
//     then copied row by row by the lane groups.
#include <type_traits>

#include "psg_ctx.h"
#include "psg_device.h"
#include "psg_rows.h"

namespace psg {
namespace {

using namespace dev;
using rows::Shape;

constexpr int kNT = rows::kThreads;
constexpr int kU = rows::kItemRows;
constexpr int kChunk = 64;  // pushes whose pieces are tabled in LDS at a time

// Device tables of a plan.  The cut and found tables hold, per job, npush
// rows of ntiles + 1 words from the job's cut0 on.
struct RowsJob {
  const uint64_t* keys;
  void* out;
  uint64_t nslots;
  uint64_t cut0;
  uint32_t npush, nne;  // pushes; non-empty pushes (kv_vector.h:177 ignores the others)
  uint32_t ntiles, tile0, push0;
  uint32_t first;  // the first non-empty push: it assigns, the others add (kv_vector.h:195-196)
};
struct RowsPush {
  const uint64_t* keys;
  const void* rows;
  uint32_t n, job;
};

template <typename V> struct Unit;
template <> struct Unit<float> { typedef float T __attribute__((ext_vector_type(4))); };
template <> struct Unit<double> { typedef double T __attribute__((ext_vector_type(2))); };

// cut(p, t) = lower_bound(S_p, D[t T]) for t < ntiles, and cut(p, ntiles) =
// upper_bound(S_p, D[nslots - 1]): keys outside D lie in no piece.
__global__ __launch_bounds__(kNT) void rows_cuts_kernel(const RowsJob* __restrict__ jobs,
                                                        const RowsPush* __restrict__ pushes,
                                                        uint32_t* __restrict__ cut, int tshift) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const RowsPush P = pushes[blockIdx.x];
  const RowsJob J = jobs[P.job];
  uint32_t* c = cut + J.cut0 + (uint64_t)(blockIdx.x - J.push0) * (J.ntiles + 1u);
  for (uint32_t t = blockIdx.y * 4u + (uint32_t)w; t <= J.ntiles; t += gridDim.y * 4u) {
    uint64_t r = 0;
    if (J.ntiles) {
      const bool last = t == J.ntiles;
      const uint64_t key = J.keys[last ? J.nslots - 1 : (uint64_t)t << tshift];
      r = wave_search(P.keys, P.n, key, last, lane);
    }
    if (lane == 0) c[t] = (uint32_t)r;
  }
}

// The rows a lane group holds for one step: the keys of its kU rows, the key
// before each (the order check) and the lane's elements of each row.
template <typename V>
struct RowRegs {
  static constexpr int E = 16 / (int)sizeof(V);
  static constexpr int NL = sizeof(V) == 8 ? rows::kMaxLoops : 1;
  uint64_t key[kU], prev[kU];
  V r[kU][NL][E];
};

template <typename V, bool kVec>
__global__ __launch_bounds__(kNT) void rows_fold_kernel(
    const RowsJob* __restrict__ jobs, const RowsPush* __restrict__ pushes,
    const uint32_t* __restrict__ tjob, const uint32_t* __restrict__ cut,
    uint32_t* __restrict__ found, int k, int parallel) {
  typedef typename Unit<V>::T VU;
  constexpr int E = RowRegs<V>::E, NL = RowRegs<V>::NL;
  static_assert(NL * 64 * E >= rows::kMaxWidth, "a lane group reaches the widest row");
  __shared__ __attribute__((aligned(16))) unsigned char lds[rows::kLdsAlloc];
  const Shape S = rows::shape_of((int)sizeof(V), k);
  const uint32_t T = (uint32_t)S.T, L = (uint32_t)S.L, NG = (uint32_t)kNT / L;  // NG lane groups
  V* const acc = (V*)lds;                                            // [T][k]
  uint64_t* const dk = (uint64_t*)(lds + (size_t)T * k * sizeof(V));  // [T]
  uint32_t* const cnt = (uint32_t*)(dk + T);                          // [T] pushes holding the slot
  // the chunk's pieces: bounds, key and row pointers; the non-empty ones; the
  // per-push matched words (two, used in turn)
  uint64_t* const m_keys = (uint64_t*)(cnt + T);
  uint64_t* const m_rows = m_keys + kChunk;
  uint64_t* const m_mask = m_rows + kChunk;
  uint32_t* const m_lo = (uint32_t*)(m_mask + 1);
  uint32_t* const m_hi = m_lo + kChunk;
  uint32_t* const pf = m_hi + kChunk;
  static_assert(kChunk * 24 + 8 + 8 <= rows::kLdsFixed, "bookkeeping");

  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = uni(tid >> 6);
  const uint32_t g = tid / L, jl = tid & (L - 1u);
  const uint32_t b = xcd_index(blockIdx.x, gridDim.x);
  const RowsJob J = jobs[tjob[b]];
  const uint32_t t = b - J.tile0;
  const uint64_t slot0 = (uint64_t)t * T;
  const uint32_t nt = J.nslots - slot0 < (uint64_t)T ? (uint32_t)(J.nslots - slot0) : T;
  const uint64_t* const Dg = J.keys + slot0;

  // ---- the tile's D into LDS: LDS-DMA for a full tile of whole waves
  const bool dma = nt == T && T >= 128u && ((uintptr_t)Dg & 15u) == 0u;
  if (dma) {
    for (uint32_t c = w; c < T / 128u; c += 4u) dma16(Dg + 128u * c + 2u * lane, (char*)dk + 1024u * c);
  } else {
    for (uint32_t s = tid; s < T; s += kNT) dk[s] = s < nt ? Dg[s] : ~0ull;
  }
  for (uint32_t s = tid; s < T; s += kNT) cnt[s] = 0u;
  if (tid < 2u) pf[tid] = 0u;

  const uint32_t* const cj = cut + J.cut0 + t;   // + p (ntiles + 1)
  uint32_t* const fj = found + J.cut0 + t;
  const uint32_t cq = J.ntiles + 1u;

  // one step's loads of this lane: rows lo + g + NG (kU it + u) of the piece
  auto load = [&](RowRegs<V>& X, uint32_t q, uint32_t it) {
    const uint64_t* Sk = (const uint64_t*)uni64(m_keys[q]);
    const V* Rw = (const V*)uni64(m_rows[q]);
    const uint32_t lo = uni(m_lo[q]), hi = uni(m_hi[q]);
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const uint64_t i = (uint64_t)lo + g + (uint64_t)NG * (kU * it + (uint32_t)u);
      const bool have = i < hi;
      X.key[u] = have ? G(Sk)[i] : 0ull;
      X.prev[u] = have && i > 0 ? G(Sk)[i - 1] : 0ull;
      const V* row = Rw + i * (uint64_t)k;
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        const uint32_t e0 = (jl + (uint32_t)l * L) * E;
        if constexpr (kVec) {
          VU x = {};
          if (have && e0 < (uint32_t)k) x = __builtin_nontemporal_load((const AS1 VU*)(row + e0));
#pragma unroll
          for (int e = 0; e < E; ++e) X.r[u][l][e] = x[e];
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e)
            X.r[u][l][e] = have && e0 + e < (uint32_t)k ? G(row)[e0 + e] : V(0);
        }
      }
    }
  };

  // one step's fold: search each row's key in the tile, then assign or add
  // (the first non-empty push assigns, fold_step's rule) the lane's elements.
  // Returns the keys found (lane jl == 0 of a group
  // votes).  A key not above the one before it is out of order: unmatched.
  auto fold = [&](const RowRegs<V>& X, uint32_t p0, uint32_t q, uint32_t it) -> uint32_t {
    const uint32_t lo = uni(m_lo[q]), hi = uni(m_hi[q]);
    const bool first = p0 + q == J.first;
    uint32_t pos[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) pos[u] = 0u;
    for (uint32_t step = T; step > 0u; step >>= 1) {  // lower_bound, kU searches abreast
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const uint32_t c = pos[u] + step;
        if (c <= nt && dk[c - 1u] < X.key[u]) pos[u] = c;
      }
    }
    uint32_t nfound = 0;
    bool hit[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const uint64_t i = (uint64_t)lo + g + (uint64_t)NG * (kU * it + (uint32_t)u);
      hit[u] = i < hi && pos[u] < nt && dk[pos[u] < nt ? pos[u] : 0u] == X.key[u] &&
               (i == 0 || X.prev[u] < X.key[u]);
      nfound += (uint32_t)__popcll(__ballot(hit[u] && jl == 0u));
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (!hit[u]) continue;
      const uint32_t s = pos[u];
      const uint32_t c = cnt[s];
      V* const a = acc + (size_t)s * k;
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        const uint32_t e0 = (jl + (uint32_t)l * L) * E;
        if constexpr (kVec) {
          if (e0 < (uint32_t)k) {
            VU x;
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = X.r[u][l][e];
            if (c || !first) {  // an untouched slot holds +0.0
              VU y = {};
              if (c) y = *(const VU*)(a + e0);
#pragma unroll
              for (int e = 0; e < E; ++e) x[e] = y[e] + x[e];
            }
            *(VU*)(a + e0) = x;
          }
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e)
            if (e0 + e < (uint32_t)k)
              a[e0 + e] = c || !first ? (c ? a[e0 + e] : V(0)) + X.r[u][l][e] : X.r[u][l][e];
        }
      }
      if (jl == 0u) cnt[s] = c + 1u;
    }
    return nfound;
  };

  uint32_t seq = 0;  // pushes folded so far: their matched word is pf[seq & 1]
  for (uint32_t p0 = 0; p0 < J.npush; p0 += kChunk) {
    // ---- the chunk's pieces (wave 0), with the matched word of empty ones
    __syncthreads();
    if (w == 0u) {
      const uint32_t p = p0 + lane;
      uint32_t lo = 0, hi = 0;
      if (p < J.npush) {
        const RowsPush P = pushes[J.push0 + p];
        lo = cj[(uint64_t)p * cq];
        hi = cj[(uint64_t)p * cq + 1u];
        hi = hi < P.n ? hi : P.n;
        if (hi <= lo) {
          hi = lo;
          fj[(uint64_t)p * cq] = 0u;
        }
        m_keys[lane] = (uint64_t)(uintptr_t)P.keys;
        m_rows[lane] = (uint64_t)(uintptr_t)P.rows;
      }
      m_lo[lane] = lo;
      m_hi[lane] = hi;
      const unsigned long long mask = __ballot(hi > lo);
      if (lane == 0u) *m_mask = mask;
    }
    if (dma && p0 == 0u) dma_wait();
    __syncthreads();
    uint64_t todo = uni64(*m_mask);
    if (!todo) continue;
    // ---- its steps, one ahead in flight
    uint32_t q = (uint32_t)__builtin_ctzll(todo), it = 0;
    RowRegs<V> cur, nxt;
    load(cur, q, it);
    uint32_t wfound = 0;
    for (;;) {
      const uint32_t len = uni(m_hi[q]) - uni(m_lo[q]);
      uint32_t nq = q, nit = it + 1u;
      if ((uint64_t)nit * (NG * kU) >= len) {  // the push's last step
        todo &= todo - 1u;
        nq = todo ? (uint32_t)__builtin_ctzll(todo) : kChunk;
        nit = 0;
      }
      if (nq < (uint32_t)kChunk) load(nxt, nq, nit);
      wfound += fold(cur, p0, q, it);
      if (nq != q) {
        // ---- the push is folded: publish before the next push's rows land
        // on the same slots, and hand its matched count to thread 0
        if (lane == 0u && wfound) atomicAdd(&pf[seq & 1u], wfound);
        lds_barrier();
        if (tid == 0u) {
          fj[(uint64_t)(p0 + q) * cq] = pf[seq & 1u];
          pf[seq & 1u] = 0u;
        }
        ++seq;
        wfound = 0;
        if (nq == (uint32_t)kChunk) break;
      }
      cur = nxt;
      q = nq;
      it = nit;
    }
  }
  if (J.npush == 0u && dma) dma_wait();
  __syncthreads();

  // ---- store: the lane groups walk the tile's rows
  V* const og = (V*)J.out + slot0 * (uint64_t)k;
  for (uint32_t s = g; s < nt; s += NG) {
    const uint32_t c = cnt[s];
    const bool gap = !parallel && c != J.nne;
    const V* const a = acc + (size_t)s * k;
    V* const o = og + (uint64_t)s * k;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const uint32_t e0 = (jl + (uint32_t)l * L) * E;
      if constexpr (kVec) {
        if (e0 < (uint32_t)k) {
          VU x = {};
          if (c) {
            x = *(const VU*)(a + e0);
            if (gap) {
#pragma unroll
              for (int e = 0; e < E; ++e) x[e] = x[e] + V(0);
            }
          }
          *(AS1 VU*)(o + e0) = x;
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (e0 + e < (uint32_t)k) {
            V x = V(0);
            if (c) x = gap ? a[e0 + e] + V(0) : a[e0 + e];
            GW(o)[e0 + e] = x;
          }
      }
    }
  }
}

// matched[p] = the keys found over the push's pieces: one wave per push
__global__ __launch_bounds__(kNT) void rows_matched_kernel(const RowsJob* __restrict__ jobs,
                                                           const RowsPush* __restrict__ pushes,
                                                           const uint32_t* __restrict__ found,
                                                           uint32_t npush,
                                                           unsigned long long* __restrict__ matched) {
  const uint32_t gp = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (gp >= npush) return;
  const RowsJob J = jobs[pushes[gp].job];
  const uint32_t* f = found + J.cut0 + (uint64_t)(gp - J.push0) * (J.ntiles + 1u);
  unsigned long long sum = 0;
  for (uint32_t t = lane; t < J.ntiles; t += 64u) sum += f[t];
  for (int d = 32; d > 0; d >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, d, 64);
  if (lane == 0u) matched[gp] = sum;
}

// ----------------------------------------------------------------------
// row gather (pull reply): out[i] = the row of req[i], or +0.0s where the
// key is absent or repeats the request before it (psg_kernels.hip's gather).
// ----------------------------------------------------------------------
template <typename V, bool kVec>
__global__ __launch_bounds__(kNT) void rows_gather_kernel(
    const uint64_t* __restrict__ D, uint64_t nd, const V* __restrict__ W,
    const uint64_t* __restrict__ req, uint64_t nreq, V* __restrict__ out,
    unsigned long long* __restrict__ matched, int k) {
  typedef typename Unit<V>::T VU;
  constexpr int E = RowRegs<V>::E, NL = RowRegs<V>::NL;
  __shared__ uint64_t rg[2];
  __shared__ uint64_t pos[kNT];
  __shared__ uint32_t wfound[kNT / 64];
  const Shape S = rows::shape_of((int)sizeof(V), k);
  const uint32_t L = (uint32_t)S.L, NG = (uint32_t)kNT / L;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const uint32_t g = tid / L, jl = tid & (L - 1u);
  const uint64_t r0 = (uint64_t)blockIdx.x * kNT;
  const uint64_t r1 = nreq - r0 < (uint64_t)kNT ? nreq : r0 + kNT;
  const uint64_t i = r0 + tid;
  const uint64_t key = i < r1 ? req[i] : 0ull;
  const uint64_t prev = i > 0 && i < r1 ? req[i - 1] : 0ull;
  if (w < 2u) {
    const uint64_t r = wave_search(D, nd, req[w == 0u ? r0 : r1 - 1], w == 1u, (int)lane);
    if (lane == 0u) rg[w] = r;
  }
  __syncthreads();
  const uint64_t lo = rg[0], hi = rg[1] > rg[0] ? rg[1] : rg[0];
  const uint64_t p = lo + gl_lower_bound(D + lo, hi - lo, key);
  const bool hit = i < r1 && p < hi && D[p] == key && !(i > 0 && prev == key);
  pos[tid] = hit ? p : ~0ull;
  const uint32_t nf = (uint32_t)__popcll(__ballot(hit));
  if (lane == 0u) wfound[w] = nf;
  __syncthreads();
  const uint32_t nr = (uint32_t)(r1 - r0);
  for (uint32_t q = g; q < nr; q += NG) {
    const uint64_t at = pos[q];
    const bool have = at != ~0ull;
    const V* const row = W + (have ? at : 0ull) * (uint64_t)k;
    V* const o = out + (r0 + q) * (uint64_t)k;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const uint32_t e0 = (jl + (uint32_t)l * L) * E;
      if constexpr (kVec) {
        if (e0 < (uint32_t)k) {
          VU x = {};
          if (have) x = *(const AS1 VU*)(row + e0);
          *(AS1 VU*)(o + e0) = x;
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (e0 + e < (uint32_t)k) GW(o)[e0 + e] = have ? G(row)[e0 + e] : V(0);
      }
    }
  }
  if (tid == 0u && matched) {
    const uint32_t tot = wfound[0] + wfound[1] + wfound[2] + wfound[3];
    if (tot) atomicAdd(matched, (unsigned long long)tot);
  }
}

template <typename F>
void by_form(int dtype, bool vec, F&& f) {
  if (dtype == PSG_F32) {
    if (vec) f(float(), std::true_type()); else f(float(), std::false_type());
  } else {
    if (vec) f(double(), std::true_type()); else f(double(), std::false_type());
  }
}

bool unit_aligned(const void* p) { return ((uintptr_t)p & (rows::kUnitBytes - 1)) == 0; }

}  // namespace
}  // namespace psg

using psg::RowsJob;
using psg::RowsPush;
namespace rows = psg::rows;

struct psg_rows_plan {
  int device = 0, dtype = 0, k = 0;
  bool parallel = false, vec = false;
  uint32_t npush = 0, ntiles = 0, cut_y = 1;
  int tshift = 0;
  RowsJob* d_jobs = nullptr;
  RowsPush* d_push = nullptr;
  uint32_t *d_tjob = nullptr, *d_cut = nullptr, *d_found = nullptr;
  unsigned long long* d_matched = nullptr;
  hipStream_t last = nullptr;
  uint64_t bytes = 0, kv = 0;
  void release() {
    (void)hipFree(d_jobs);
    (void)hipFree(d_push);
    (void)hipFree(d_tjob);
    (void)hipFree(d_cut);
    (void)hipFree(d_found);
    (void)hipFree(d_matched);
  }
};

namespace {
template <typename T>
int upload(T** dst, const std::vector<T>& src, size_t count) {
  HIP_TRY(hipMalloc((void**)dst, sizeof(T) * std::max<size_t>(1, count)));
  if (!src.empty())
    HIP_TRY(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return PSG_OK;
}
}  // namespace

extern "C" {

int psg_rows_max_width(void) { return rows::kMaxWidth; }

int psg_rows_shape(int dtype, int k, int shape[4]) {
  if (!shape || (dtype != PSG_F32 && dtype != PSG_F64) || !rows::valid((int)psg::vsize(dtype), k))
    return psg::fail(PSG_ERR_ARG, "rows: dtype %d, k %d", dtype, k);
  const rows::Shape s = rows::shape_of((int)psg::vsize(dtype), k);
  shape[0] = s.T;
  shape[1] = s.L;
  shape[2] = s.E;
  shape[3] = s.R;
  return PSG_OK;
}

int psg_rows_plan_create(int device, int dtype, int k, unsigned flags, const psg_rows_job* jobs,
                         int njobs, psg_rows_plan** out) {
  using psg::fail;
  if (!out || njobs < 0 || (njobs > 0 && !jobs)) return fail(PSG_ERR_ARG, "null argument");
  if (dtype != PSG_F32 && dtype != PSG_F64) return fail(PSG_ERR_ARG, "dtype %d", dtype);
  if (flags & ~PSG_PARALLEL_MATCH) return fail(PSG_ERR_ARG, "rows: flags %#x", flags);
  const int sv = (int)psg::vsize(dtype);
  if (!rows::valid(sv, k)) return fail(PSG_ERR_ARG, "rows: k=%d", k);
  const rows::Shape S = rows::shape_of(sv, k);
  std::vector<RowsJob> hj(njobs);
  std::vector<RowsPush> hp;
  std::vector<uint32_t> tjob;
  uint64_t ncut = 0, bytes = 0, kv = 0, maxcuts = 1;
  bool vec = (k * sv) % rows::kUnitBytes == 0;
  for (int j = 0; j < njobs; ++j) {
    const psg_rows_job& J = jobs[j];
    if (J.npush < 0 || J.npush > psg::kMaxPush) return fail(PSG_ERR_ARG, "job %d: npush=%d", j, J.npush);
    if ((J.npush > 0 && (!J.push_keys || !J.push_rows || !J.push_n)) ||
        (J.nslots > 0 && (!J.keys || !J.out)))
      return fail(PSG_ERR_ARG, "job %d: null pointer", j);
    const uint64_t ntiles = (J.nslots + S.T - 1) / S.T;
    if (ntiles + tjob.size() >= (1ull << 31)) return fail(PSG_ERR_ARG, "job %d: too many tiles", j);
    RowsJob& h = hj[j];
    h.keys = J.keys;
    h.out = J.out;
    h.nslots = J.nslots;
    h.cut0 = ncut;
    h.npush = (uint32_t)J.npush;
    h.nne = 0;
    h.ntiles = (uint32_t)ntiles;
    h.tile0 = (uint32_t)tjob.size();
    h.push0 = (uint32_t)hp.size();
    h.first = ~0u;
    vec = vec && psg::unit_aligned(J.out);
    for (int p = 0; p < J.npush; ++p) {
      const uint64_t n = J.push_n[p];
      if (n >= (1ull << 32)) return fail(PSG_ERR_ARG, "job %d push %d: n >= 2^32", j, p);
      if (n > 0 && (!J.push_keys[p] || !J.push_rows[p]))
        return fail(PSG_ERR_ARG, "job %d push %d: null pointer", j, p);
      hp.push_back(RowsPush{J.push_keys[p], J.push_rows[p], (uint32_t)n, (uint32_t)j});
      if (n > 0 && h.nne++ == 0) h.first = (uint32_t)p;
      vec = vec && psg::unit_aligned(J.push_rows[p]);
      bytes += n * (8 + (uint64_t)k * sv);
      kv += n;
    }
    bytes += J.nslots * (8 + (uint64_t)k * sv);
    ncut += (uint64_t)J.npush * (ntiles + 1);
    maxcuts = std::max(maxcuts, ntiles + 1);
    tjob.insert(tjob.end(), (size_t)ntiles, (uint32_t)j);
  }
  if (int rc = psg::set_dev(device)) return rc;
  psg_rows_plan* P = new psg_rows_plan();
  P->device = device;
  P->dtype = dtype;
  P->k = k;
  P->parallel = (flags & PSG_PARALLEL_MATCH) != 0;
  P->vec = vec;
  P->npush = (uint32_t)hp.size();
  P->ntiles = (uint32_t)tjob.size();
  P->cut_y = (uint32_t)std::min<uint64_t>((maxcuts + 3) / 4, 4096);
  while ((1 << P->tshift) < S.T) ++P->tshift;
  P->bytes = bytes;
  P->kv = kv;
  int rc = upload(&P->d_jobs, hj, hj.size());
  if (!rc) rc = upload(&P->d_push, hp, hp.size());
  if (!rc) rc = upload(&P->d_tjob, tjob, tjob.size());
  if (!rc) rc = upload(&P->d_cut, std::vector<uint32_t>(), ncut);
  if (!rc) rc = upload(&P->d_found, std::vector<uint32_t>(), ncut);
  if (!rc) rc = upload(&P->d_matched, std::vector<unsigned long long>(), hp.size());
  if (rc) {
    P->release();
    delete P;
    return rc;
  }
  *out = P;
  return PSG_OK;
}

int psg_rows_plan_run(psg_rows_plan* P, void* stream) {
  if (!P) return psg::fail(PSG_ERR_ARG, "null plan");
  hipStream_t s = (hipStream_t)stream;
  P->last = s;
  if (P->npush)
    hipLaunchKernelGGL(psg::rows_cuts_kernel, dim3(P->npush, P->cut_y), dim3(psg::kNT), 0, s,
                       P->d_jobs, P->d_push, P->d_cut, P->tshift);
  if (P->ntiles)
    psg::by_form(P->dtype, P->vec, [&](auto v, auto vec) {
      hipLaunchKernelGGL((psg::rows_fold_kernel<decltype(v), decltype(vec)::value>), dim3(P->ntiles),
                         dim3(psg::kNT), 0, s, P->d_jobs, P->d_push, P->d_tjob, P->d_cut,
                         P->d_found, P->k, (int)P->parallel);
    });
  HIP_TRY(hipGetLastError());
  return PSG_OK;
}

int psg_rows_plan_matched(psg_rows_plan* P, uint64_t* matched) {
  if (!P || !matched) return psg::fail(PSG_ERR_ARG, "null argument");
  if (int rc = psg::set_dev(P->device)) return rc;
  if (!P->npush) return PSG_OK;
  hipLaunchKernelGGL(psg::rows_matched_kernel, dim3((P->npush + 3) / 4), dim3(psg::kNT), 0, P->last,
                     P->d_jobs, P->d_push, P->d_found, P->npush, P->d_matched);
  HIP_TRY(hipGetLastError());
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "matched words");
  HIP_TRY(hipMemcpyAsync(matched, P->d_matched, 8 * (size_t)P->npush, hipMemcpyDeviceToHost,
                         P->last));
  HIP_TRY(hipStreamSynchronize(P->last));
  return PSG_OK;
}

int psg_rows_plan_bytes(psg_rows_plan* P, uint64_t* bytes, uint64_t* kv) {
  if (!P) return psg::fail(PSG_ERR_ARG, "null plan");
  if (bytes) *bytes = P->bytes;
  if (kv) *kv = P->kv;
  return PSG_OK;
}

int psg_rows_plan_destroy(psg_rows_plan* P) {
  if (!P) return PSG_OK;
  (void)hipSetDevice(P->device);
  P->release();
  delete P;
  return PSG_OK;
}

int psg_gather_rows_dev(int dtype, int k, const uint64_t* dkeys, uint64_t nd, const void* drows,
                        const uint64_t* req, uint64_t nreq, void* out,
                        unsigned long long* matched, void* stream) {
  if (dtype != PSG_F32 && dtype != PSG_F64) return psg::fail(PSG_ERR_ARG, "dtype %d", dtype);
  const int sv = (int)psg::vsize(dtype);
  if (!rows::valid(sv, k)) return psg::fail(PSG_ERR_ARG, "rows: k=%d", k);
  if (nreq == 0) return PSG_OK;
  if (!req || !out || (nd > 0 && (!dkeys || !drows))) return psg::fail(PSG_ERR_ARG, "null argument");
  const uint64_t blocks = (nreq + psg::kNT - 1) / psg::kNT;
  if (blocks >= (1ull << 31)) return psg::fail(PSG_ERR_ARG, "rows: nreq");
  const bool vec = (k * sv) % rows::kUnitBytes == 0 && psg::unit_aligned(drows) &&
                   psg::unit_aligned(out);
  psg::by_form(dtype, vec, [&](auto v, auto vf) {
    typedef decltype(v) V;
    hipLaunchKernelGGL((psg::rows_gather_kernel<V, decltype(vf)::value>), dim3((uint32_t)blocks),
                       dim3(psg::kNT), 0, (hipStream_t)stream, dkeys, nd, (const V*)drows, req,
                       nreq, (V*)out, matched, k);
  });
  HIP_TRY(hipGetLastError());
  return PSG_OK;
}

}  // extern "C"
