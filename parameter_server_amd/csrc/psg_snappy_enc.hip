// psg_snappy_enc.hip -- snappy raw-format compression of device-resident
// message parts: what Van::send does per key and value part
// (system/van.cc:121-131, SArray::compressTo, base/shared_array_inl.h:244-256)
// for the arrays the device now produces.  The stream of a part is a pure
// function of its bytes: psg_snappy_enc.h's rule, which psg_snappy_enc.cc
// walks serially on the host with the same result.
//
// Three launches, none of which waits on another workgroup:
//   setup   one workgroup: the parts' fragment counts, scanned (fbase)
//   encode  one workgroup of 256 threads per 64 KB fragment: the fragment
//           and its hash table live in LDS (64 + 64 KB, so one workgroup per
//           CU, a wave on every SIMD); a step's 256 positions are one lane
//           each for the lookup and the insert, wave 0 selects; the stream
//           goes to the fragment's worst-case slot
//   pack    one workgroup per fragment: the lengths of the part's earlier
//           fragments summed, the slot copied behind them in the part's
//           stream; the preamble and clen[i]
// The host knows neither the parts' sizes nor their fragment count (soff is
// a device array and nothing waits), so encode and pack run a fixed grid
// whose workgroups stride over the fragments; a workgroup without one ends
// at once.
#include <hip/hip_runtime.h>

#include "psg_device.h"
#include "psg_host.h"
#include "psg_internal.h"
#include "psg_snappy_enc.h"

namespace psg {
namespace {

using namespace snappy_enc;

constexpr uint32_t kThreads = kStep;  // one lane per position of a step
constexpr uint32_t kMaxEl = kStep / kMinMatch;  // copies selected in one step
constexpr uint32_t kShortLit = 16;              // a literal its element's lane writes itself
// a step's longer literals: but for the first, each lies in the step with
// its copy, kShortLit + 1 + kMinMatch positions or more
constexpr uint32_t kMaxLong = kStep / (kShortLit + 1 + kMinMatch) + 1;
constexpr uint32_t kGrid = 1024;                // 4 workgroups per CU over a long input
constexpr uint64_t kMaxPart = 0xffffffffull;    // the preamble is a 32-bit varint

// scratch: fbase[nparts + 1] | flen[nfrag] | slots[nfrag][kSlot]
__host__ __device__ inline uint64_t align_to(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
__host__ __device__ inline uint64_t flen_offset(uint64_t nparts) {
  return align_to(8 * (nparts + 1), 16);
}
__host__ __device__ inline uint64_t slots_offset(uint64_t nparts, uint64_t nfrag) {
  return align_to(flen_offset(nparts) + 4 * nfrag, 256);
}

__device__ inline uint64_t part_fragments(uint64_t n) { return n > kMaxPart ? 0 : fragments_of(n); }

// fbase[i]: the fragments of the parts before i.  One workgroup; every loop
// is bounded by nparts.
__global__ __launch_bounds__(kThreads) void snappy_enc_setup_kernel(
    const uint64_t* __restrict__ soff, uint64_t nparts, uint64_t* __restrict__ clen,
    uint64_t* __restrict__ fbase) {
  __shared__ uint64_t sum[kThreads];
  const uint32_t tid = threadIdx.x;
  const uint64_t chunk = (nparts + kThreads - 1) / kThreads;
  const uint64_t lo = min(tid * chunk, nparts), hi = min(lo + chunk, nparts);
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t n = soff[i + 1] - soff[i];
    if (n > kMaxPart) clen[i] = 0;  // no stream: not a part snappy can declare
    s += part_fragments(n);
  }
  sum[tid] = s;
  __syncthreads();
  if (tid == 0) {
    uint64_t run = 0;
    for (uint32_t t = 0; t < kThreads; ++t) {
      const uint64_t x = sum[t];
      sum[t] = run;
      run += x;
    }
    fbase[nparts] = run;
  }
  __syncthreads();
  uint64_t run = sum[tid];
  for (uint64_t i = lo; i < hi; ++i) {
    fbase[i] = run;
    run += part_fragments(soff[i + 1] - soff[i]);
  }
}

// the part that fragment f < fbase[nparts] belongs to: the i with
// fbase[i] <= f < fbase[i + 1]
__device__ inline uint64_t part_of(const uint64_t* __restrict__ fbase, uint64_t nparts,
                                   uint64_t f) {
  uint64_t lo = 0, hi = nparts - 1;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (fbase[mid + 1] <= f) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void snappy_enc_kernel(
    const uint8_t* __restrict__ src, const uint64_t* __restrict__ soff, uint64_t nparts,
    uint8_t* __restrict__ scratch) {
  __shared__ uint32_t frag[kFragment / 4 + 4];  // the fragment's bytes, and a word of slack
  __shared__ uint32_t T[1u << kHashBits];       // hash -> the largest earlier position + 1
  __shared__ uint32_t M[kStep];                 // this step's matches (pack_match)
  // the elements a step selects: the literal's start, the copy's position,
  // its match and the element's place in the slot; those with a long literal
  __shared__ uint32_t el_lit[kMaxEl], el_p[kMaxEl], el_m[kMaxEl], el_o[kMaxEl], el_long[kMaxLong];
  __shared__ uint32_t s_ne, s_nl, s_lit, s_o;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint8_t* frag8 = (const uint8_t*)frag;
  const auto ld = [&](uint32_t x) {
    const uint32_t w = x >> 2;
    return (uint32_t)(((uint64_t)frag[w + 1] << 32 | frag[w]) >> (8 * (x & 3u)));
  };
  const uint64_t* fbase = (const uint64_t*)scratch;
  const uint64_t total = fbase[nparts];
  uint32_t* flen = (uint32_t*)(scratch + flen_offset(nparts));
  uint8_t* slots = scratch + slots_offset(nparts, total);
  for (uint64_t f = blockIdx.x; f < total; f += gridDim.x) {
    const uint64_t i = part_of(fbase, nparts, f);
    const uint64_t n = soff[i + 1] - soff[i], b = (f - fbase[i]) * kFragment;
    const uint32_t L = (uint32_t)min((uint64_t)kFragment, n - b);
    uint8_t* d = slots + f * kSlot;
    {
      // the fragment into LDS by aligned words: only words that hold a byte
      // of the fragment are read
      const uint8_t* s = src + soff[i] + b;
      const uint32_t a = (uint32_t)((uintptr_t)s & 3u);
      const uint32_t* g = (const uint32_t*)(s - a);
      const uint32_t nin = (a + L + 3) / 4;
      for (uint32_t w = tid; w < kFragment / 4 + 4; w += kThreads) {
        uint32_t v = 0;
        if (w * 4 < L) {
          const uint32_t lo = g[w], hi = (a && w + 1 < nin) ? g[w + 1] : 0u;
          v = (uint32_t)(((uint64_t)hi << 32 | lo) >> (8 * a));
        }
        frag[w] = v;
      }
      for (uint32_t h = tid; h < (1u << kHashBits); h += kThreads) T[h] = 0;
    }
    __syncthreads();
    uint32_t q = 0, lit = 0, o = 0;  // wave 0's: the cursor, the last copy's end, bytes out
    for (uint32_t base = 0; base < L; base += kStep) {
      // 1. lookup
      const uint32_t p = base + tid;
      const bool live = p + 4 <= L;
      uint32_t h = 0, m = 0;
      if (live) {
        h = hash(ld(p));
        const uint32_t e = T[h];
        if (e) {
          const uint32_t len = match_len(ld, e - 1, p, min(kMaxCopy, L - p));
          if (len >= kMinMatch) m = pack_match(len, p - (e - 1));
        }
      }
      M[tid] = m;
      __syncthreads();
      // 2. insert
      if (live) atomicMax(&T[h], p + 1);
      // 3. select, by wave 0, 64 positions at a time, a lane each.  The walk
      // from match to match runs on wave-uniform values (the ballot of the
      // lanes that hold a match, one readlane per copy); the elements it
      // picks are then sized, scanned into output offsets and listed in
      // parallel
      if (wave == 0) {
        const uint32_t end = min(base + kStep, L);
        uint32_t ne = 0, nl = 0;
        for (uint32_t cb = base; cb < end; cb += 64) {
          const uint32_t mv = M[cb - base + lane], len = mv >> 16;
          const unsigned long long has = __ballot(mv != 0);
          // the walk, relative to cb: from the cursor to the first lane
          // that holds a match, from there to its copy's end, and so on; at
          // most 16 copies, each moves the cursor on by 4 or more
          const uint32_t rel_end = lane + len;
          const uint32_t start = max(q, cb) - cb;
          unsigned long long open = start < 64 ? has & (~0ull << start) : 0, sel = 0;
          uint32_t stop = 0;
          while (open) {
            const uint32_t r = (uint32_t)__builtin_ctzll(open);
            sel |= 1ull << r;
            stop = (uint32_t)__builtin_amdgcn_readlane((int)rel_end, (int)r);
            open = stop < 64 ? open & (~0ull << stop) : 0;
          }
          q = cb + max(stop, 64u);
          if (sel) {
            const bool mine = (sel >> lane) & 1u;
            const unsigned long long below = sel & ((1ull << lane) - 1);
            const uint32_t pos = cb + lane, my_end = pos + len;
            // the literal in front of my copy starts where the copy selected
            // before it ends
            const uint32_t before = (uint32_t)__shfl((int)my_end, below ? 63 - __builtin_clzll(below) : 0);
            const uint32_t l0 = below ? before : lit, r = pos - l0;
            const uint32_t sz = mine ? (r ? literal_header_len(r) + r : 0) + copy_len(len, mv & 0xffffu) : 0;
            const uint32_t incl = dev::wave_scan_incl(sz);
            const uint32_t e = ne + (uint32_t)__builtin_popcountll(below);
            if (mine) {
              el_lit[e] = l0;
              el_p[e] = pos;
              el_m[e] = mv;
              el_o[e] = o + incl - sz;
            }
            const bool lg = mine && r > kShortLit;
            const unsigned long long lb = __ballot(lg);
            if (lg) el_long[nl + (uint32_t)__builtin_popcountll(lb & ((1ull << lane) - 1))] = e;
            nl += (uint32_t)__builtin_popcountll(lb);
            ne += (uint32_t)__builtin_popcountll(sel);
            lit = (uint32_t)__builtin_amdgcn_readlane((int)my_end, 63 - __builtin_clzll(sel));
            o += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
          }
        }
        if (lane == 0) {
          s_ne = ne;
          s_nl = nl;
        }
      }
      __syncthreads();
      // the step's elements, a lane each: the tags, and a literal of up to
      // kShortLit bytes; the longer literals by all threads
      const uint32_t ne = s_ne, nl = s_nl;
      if (tid < ne) {
        const uint32_t l0 = el_lit[tid], r = el_p[tid] - l0, mv = el_m[tid];
        uint8_t* w = d + el_o[tid];
        if (r) {
          const uint32_t hl = put_literal_header(w, r);
          if (r <= kShortLit)
            for (uint32_t k = 0; k < r; ++k) w[hl + k] = frag8[l0 + k];
          w += hl + r;
        }
        put_copy(w, mv >> 16, mv & 0xffffu);
      }
      for (uint32_t j = 0; j < nl; ++j) {
        const uint32_t e = el_long[j], l0 = el_lit[e], r = el_p[e] - l0;
        uint8_t* w = d + el_o[e] + literal_header_len(r);
        for (uint32_t k = tid; k < r; k += kThreads) w[k] = frag8[l0 + k];
      }
    }
    if (tid == 0) {  // wave 0 holds the walk's state
      s_lit = lit;
      s_o = o;
    }
    __syncthreads();
    {
      // the literal at the fragment's end
      const uint32_t l0 = s_lit, r = L - l0;
      uint32_t out = s_o;
      if (r) {
        const uint32_t hl = literal_header_len(r);
        uint8_t* w = d + out;
        if (tid == 0) put_literal_header(w, r);
        for (uint32_t k = tid; k < r; k += kThreads) w[hl + k] = frag8[l0 + k];
        out += hl + r;
      }
      if (tid == 0) flen[f] = out;
    }
    __syncthreads();  // LDS is reused by the next fragment
  }
}

__global__ __launch_bounds__(kThreads) void snappy_enc_pack_kernel(
    const uint64_t* __restrict__ soff, uint64_t nparts, const uint8_t* __restrict__ scratch,
    uint8_t* __restrict__ dst, const uint64_t* __restrict__ doff, uint64_t* __restrict__ clen) {
  __shared__ unsigned long long acc;
  const uint32_t tid = threadIdx.x;
  const uint64_t* fbase = (const uint64_t*)scratch;
  const uint64_t total = fbase[nparts];
  const uint32_t* flen = (const uint32_t*)(scratch + flen_offset(nparts));
  const uint8_t* slots = scratch + slots_offset(nparts, total);
  for (uint64_t f = blockIdx.x; f < total; f += gridDim.x) {
    const uint64_t i = part_of(fbase, nparts, f);
    const uint64_t f0 = fbase[i], j = f - f0, n = soff[i + 1] - soff[i];
    // where the fragment's stream starts: behind the preamble and the
    // streams of the part's j earlier fragments
    if (tid == 0) acc = 0;
    __syncthreads();
    unsigned long long s = 0;
    for (uint64_t k = tid; k < j; k += kThreads) s += flen[f0 + k];
    if (s) atomicAdd(&acc, s);
    __syncthreads();
    const uint64_t o = varint_len((uint32_t)n) + acc;
    __syncthreads();  // acc is reset by the next fragment
    const uint32_t len = flen[f];
    uint8_t* w = dst + doff[i];
    if (tid == 0) {
      if (j == 0) put_varint(w, (uint32_t)n);
      if (f + 1 == fbase[i + 1]) clen[i] = o + len;
    }
    // slot -> stream: bytes up to the stream's next word boundary, whole
    // words (the slot is word-aligned, the stream need not be), the rest
    w += o;
    const uint32_t* sw = (const uint32_t*)(slots + f * kSlot);
    const uint8_t* sb = (const uint8_t*)sw;
    const uint32_t head = min((uint32_t)(-(uintptr_t)w & 3u), len);
    const uint32_t nw = (len - head) / 4, tail = head + 4 * nw;
    if (tid < head) w[tid] = sb[tid];
    uint32_t* ww = (uint32_t*)(w + head);
    for (uint32_t k = tid; k < nw; k += kThreads) {
      // the slot's bytes head + 4k .. + 3: at most kSlot / 4 - 1 is read,
      // since len <= kSlot - 8
      const uint32_t x = head + 4 * k, q = x >> 2;
      ww[k] = (uint32_t)(((uint64_t)sw[q + 1] << 32 | sw[q]) >> (8 * (x & 3u)));
    }
    if (tid < len - tail) w[tail + tid] = sb[tail + tid];
  }
}

}  // namespace

size_t snappy_compress_scratch_bytes(size_t total_src_bytes, uint64_t nparts) {
  // a part of n bytes has at most n / kFragment + 1 fragments
  const uint64_t nfrag = total_src_bytes / kFragment + nparts;
  return (size_t)(slots_offset(nparts, nfrag) + nfrag * kSlot);
}

hipError_t launch_snappy_compress(const uint8_t* src, const uint64_t* soff, uint64_t nparts,
                                  uint8_t* dst, const uint64_t* doff, uint64_t* clen,
                                  void* scratch, hipStream_t stream) {
  if (nparts == 0) return hipSuccess;
  hipLaunchKernelGGL(snappy_enc_setup_kernel, dim3(1), dim3(kThreads), 0, stream, soff, nparts,
                     clen, (uint64_t*)scratch);
  hipLaunchKernelGGL(snappy_enc_kernel, dim3(kGrid), dim3(kThreads), 0, stream, src, soff, nparts,
                     (uint8_t*)scratch);
  hipLaunchKernelGGL(snappy_enc_pack_kernel, dim3(kGrid), dim3(kThreads), 0, stream, soff, nparts,
                     (const uint8_t*)scratch, dst, doff, clen);
  return hipGetLastError();
}

}  // namespace psg
