// psg_snappy_enc.cc -- the host twin of the device snappy encoder
// (DESIGN.md 4.12): psg_snappy_enc.h's rule walked serially, one fragment
// after the other.  It gives the stream of psg_snappy_compress_dev byte for
// byte, so the encoder can be checked against a real snappy decoder on a
// machine without a GPU.  Host code only: no HIP call.
#include "psg_snappy_enc.h"

#include <string.h>

#include <algorithm>
#include <vector>

#include "psg_host.h"

namespace psg {
namespace snappy_enc {
namespace {

// the stream of the fragment s[0, L) at d (kSlot bytes at the most); its length
uint32_t encode_fragment(const uint8_t* s, uint32_t L, uint8_t* d, std::vector<uint32_t>& T) {
  std::fill(T.begin(), T.end(), 0u);
  auto ld = [s, L](uint32_t x) {
    uint32_t v = 0;
    if (x < L) memcpy(&v, s + x, std::min(4u, L - x));
    return v;
  };
  uint32_t M[kStep];
  uint32_t q = 0, lit = 0, o = 0;  // the cursor, the end of the last copy, bytes written
  for (uint32_t base = 0; base < L; base += kStep) {
    const uint32_t end = std::min(base + kStep, L);
    for (uint32_t p = base; p < end; ++p) {  // 1. lookup
      uint32_t m = 0;
      const uint32_t e = p + 4 <= L ? T[hash(ld(p))] : 0;
      if (e) {
        const uint32_t len = match_len(ld, e - 1, p, std::min(kMaxCopy, L - p));
        if (len >= kMinMatch) m = pack_match(len, p - (e - 1));
      }
      M[p - base] = m;
    }
    for (uint32_t p = base; p < end && p + 4 <= L; ++p) {  // 2. insert
      uint32_t& t = T[hash(ld(p))];
      t = std::max(t, p + 1);
    }
    uint32_t p = std::max(q, base);
    while (p < end) {  // 3. select
      const uint32_t m = M[p - base];
      if (!m) {
        ++p;
        continue;
      }
      if (p > lit) {
        o += put_literal_header(d + o, p - lit);
        memcpy(d + o, s + lit, p - lit);
        o += p - lit;
      }
      o += put_copy(d + o, m >> 16, m & 0xffffu);
      p += m >> 16;
      lit = p;
    }
    q = p;
  }
  if (L > lit) {
    o += put_literal_header(d + o, L - lit);
    memcpy(d + o, s + lit, L - lit);
    o += L - lit;
  }
  return o;
}

}  // namespace
}  // namespace snappy_enc
}  // namespace psg

extern "C" size_t psg_snappy_max_compressed_length(size_t n) {
  return psg::snappy_enc::max_compressed_length(n);
}

extern "C" int psg_snappy_compress_host(const void* src, size_t n, void* dst, size_t cap,
                                        size_t* len) {
  using namespace psg::snappy_enc;
  if (!dst || !len || (n && !src)) return psg::fail(PSG_ERR_ARG, "null argument");
  if (n > 0xffffffffull)  // the preamble is a varint of at most 32 bits
    return psg::fail(PSG_ERR_SIZE, "snappy: a part of %zu bytes", n);
  if (cap < max_compressed_length(n))
    return psg::fail(PSG_ERR_SIZE, "snappy: room for %zu bytes, a part of %zu may need %zu", cap, n,
                     max_compressed_length(n));
  const uint8_t* s = (const uint8_t*)src;
  uint8_t* d = (uint8_t*)dst;
  size_t o = put_varint(d, (uint32_t)n);
  std::vector<uint32_t> T(size_t(1) << kHashBits);
  std::vector<uint8_t> slot(kSlot);
  for (size_t b = 0; b < n; b += kFragment) {
    const uint32_t flen = encode_fragment(s + b, (uint32_t)std::min<size_t>(kFragment, n - b),
                                          slot.data(), T);
    memcpy(d + o, slot.data(), flen);
    o += flen;
  }
  *len = o;
  return PSG_OK;
}
