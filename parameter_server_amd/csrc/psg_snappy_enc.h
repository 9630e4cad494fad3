// psg_snappy_enc.h -- the snappy encoder's rule: what the
// stream of an input is, down to the byte.  The same code runs in the kernels
// (psg_snappy_enc.hip), in the host twin (psg_snappy_enc.cc) and in
// tests/cpp/test_snappy_enc.cc, so the two encoders cannot drift apart in a
// tag, a length form or the hash.
//
// The stream is the raw snappy format Van::send puts on the wire through
// SArray::compressTo (system/van.cc:121-131, base/shared_array_inl.h:244-256):
// a varint preamble of the uncompressed length, then literal, copy-1 and
// copy-2 elements.  The input is cut into fragments of kFragment bytes, each
// parsed on its own (no copy reaches before its fragment's start, so every
// offset is below 65536 and copy-4 never appears).
//
// One fragment of L bytes, positions 0 .. L - 1, is walked in steps of kStep
// positions; step t holds [t * kStep, min((t + 1) * kStep, L)).  A table T of
// 2^kHashBits entries, empty at the fragment's start, is keyed by
// hash(the 4 bytes at p), for the positions p with p + 4 <= L.  Per step, in
// this order:
//   1. lookup: every position p of the step with p + 4 <= L reads c = T[hash];
//      c is a position of an EARLIER step.  m(p) = the number of equal bytes
//      at c + k and p + k for k < min(kMaxCopy, L - p).  p holds a match
//      (offset p - c, length m(p)) if m(p) >= kMinMatch.
//   2. insert: T[hash] = max(T[hash], p) for every such p of the step -- by
//      max, so the order of the inserts does not matter.
//   3. select: a cursor q (0 at the fragment's start) walks the step from
//      max(q, the step's first position): at the first p >= q that holds a
//      match, the bytes [the end of the last copy, p) go out as one literal
//      (none if empty), the match as one copy, and q = p + m(p); q may pass
//      the step's end.  Without a match the cursor moves on by one.
// After the last step the bytes behind the last copy go out as one literal.
// A copy of 4 .. 11 bytes at an offset below 2048 is a copy-1, every other a
// copy-2.  A match is never longer than kMaxCopy = 64 bytes, so a long repeat
// comes out as consecutive 64-byte copies, each found by its own position.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PSG_HD __host__ __device__ inline
#else
#define PSG_HD inline
#endif

namespace psg {
namespace snappy_enc {

constexpr uint32_t kFragment = 65536;  // snappy's kBlockSize
constexpr uint32_t kStep = 256;        // positions per step
constexpr uint32_t kHashBits = 14;     // snappy's largest table (kMaxHashTableBits)
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kMaxCopy = 64;
// a table entry holds p + 1; 0: no position has reached it

// A fragment's stream is never longer than this: a literal of r bytes costs
// r + 1 (r <= 60), r + 2 (r <= 256) or r + 3 bytes, a copy of >= 4 bytes at
// most 3.  A literal and the copy behind it are thus at most 2 bytes longer
// than their input, and only where the literal has 257 bytes or more (1 byte
// from 61 on): below L / 65 over a fragment, plus 3 for the literal at its
// end.
constexpr uint32_t kSlot = kFragment + 2048;

// snappy::MaxCompressedLength
PSG_HD size_t max_compressed_length(size_t n) { return 32 + n + n / 6; }

PSG_HD uint64_t fragments_of(uint64_t n) { return n ? (n + kFragment - 1) / kFragment : 1; }

PSG_HD uint32_t hash(uint32_t bytes4) { return (bytes4 * 0x1e35a7bdu) >> (32 - kHashBits); }

PSG_HD uint32_t varint_len(uint32_t n) {
  return n < (1u << 7) ? 1 : n < (1u << 14) ? 2 : n < (1u << 21) ? 3 : n < (1u << 28) ? 4 : 5;
}
PSG_HD uint32_t put_varint(uint8_t* d, uint32_t n) {
  uint32_t i = 0;
  for (; n >= 0x80; n >>= 7) d[i++] = (uint8_t)(n | 0x80);
  d[i++] = (uint8_t)n;
  return i;
}

// the tag and length bytes in front of a literal of r >= 1 bytes (r <= kFragment)
PSG_HD uint32_t literal_header_len(uint32_t r) { return r <= 60 ? 1 : r <= 256 ? 2 : 3; }
PSG_HD uint32_t put_literal_header(uint8_t* d, uint32_t r) {
  const uint32_t n = r - 1;
  if (r <= 60) {
    d[0] = (uint8_t)(n << 2);
    return 1;
  }
  if (r <= 256) {
    d[0] = 60 << 2;
    d[1] = (uint8_t)n;
    return 2;
  }
  d[0] = 61 << 2;
  d[1] = (uint8_t)n;
  d[2] = (uint8_t)(n >> 8);
  return 3;
}

// a copy of kMinMatch <= len <= kMaxCopy bytes at 1 <= off < 65536
PSG_HD uint32_t copy_len(uint32_t len, uint32_t off) { return len <= 11 && off < 2048 ? 2 : 3; }
PSG_HD uint32_t put_copy(uint8_t* d, uint32_t len, uint32_t off) {
  if (len <= 11 && off < 2048) {
    d[0] = (uint8_t)(1 | (len - 4) << 2 | (off >> 8) << 5);
    d[1] = (uint8_t)off;
    return 2;
  }
  d[0] = (uint8_t)(2 | (len - 1) << 2);
  d[1] = (uint8_t)off;
  d[2] = (uint8_t)(off >> 8);
  return 3;
}

// m(p) of step 1 above: ld(x) gives the bytes x .. x + 3 of the fragment as
// a little-endian word; what it gives for a byte at or past the fragment's
// end is never looked at
template <class Load>
PSG_HD uint32_t match_len(Load ld, uint32_t c, uint32_t p, uint32_t lim) {
  for (uint32_t k = 0; k < lim; k += 4) {
    const uint32_t x = ld(c + k) ^ ld(p + k);
    if (x) {
      k += (uint32_t)__builtin_ctz(x) >> 3;
      return k < lim ? k : lim;
    }
  }
  return lim;
}

// What a position holds after step 1, in one word: 0 for no match
PSG_HD uint32_t pack_match(uint32_t len, uint32_t off) { return len << 16 | off; }

}  // namespace snappy_enc
}  // namespace psg
