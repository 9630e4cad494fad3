// psg_snappy_compress_host (parameter_server_amd/csrc/psg_snappy_enc.cc) on
// the encoder's edge inputs, as a stand-alone host program
// (tests/test_snappy_compress_cpp.py builds it with plain g++ under the
// address and undefined-behaviour sanitizers).  The source is a heap buffer
// of the exact length; the destination is a heap buffer of exactly the
// maximum compressed length (so the sanitizer sees a byte written past it),
// and once more with a guard pattern behind that length inside the buffer.
// Every stream is decoded here by a plain decoder and must give the input.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/psg.h"
#include "../../parameter_server_amd/csrc/psg_host.h"
#include "../../parameter_server_amd/csrc/psg_snappy_enc.h"

static int g_bad = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      if (++g_bad <= 20) printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                          \
  } while (0)

int psg::fail(int code, const char* fmt, ...) {
  (void)fmt;
  return code;
}

using namespace psg::snappy_enc;
typedef std::vector<uint8_t> Bytes;

static uint64_t g_state = 0;
static uint64_t splitmix64() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static Bytes random_bytes(uint64_t seed, size_t n) {
  g_state = seed;
  Bytes b(n);
  for (size_t i = 0; i < n; ++i) b[i] = (uint8_t)(splitmix64() >> 56);
  return b;
}
static Bytes periodic(size_t n, size_t period) {
  Bytes b(n);
  for (size_t i = 0; i < n; ++i) b[i] = (uint8_t)('A' + i % period);
  return b;
}
// `lead` random bytes, bytes [from, from + m) of them again, a byte that
// differs, a random tail
static Bytes repeat(uint64_t seed, size_t lead, size_t from, size_t m) {
  Bytes b = random_bytes(seed, lead);
  b.insert(b.end(), b.begin() + from, b.begin() + from + m);
  b.push_back((uint8_t)(b[from + m] ^ 0xFF));
  const Bytes t = random_bytes(seed + 1, 20);
  b.insert(b.end(), t.begin(), t.end());
  return b;
}

// a plain decoder of the raw format: false for anything out of bounds
static bool decode(const uint8_t* s, size_t n, Bytes* out, bool* copy4, uint32_t* max_off) {
  size_t p = 0;
  uint64_t ulen = 0;
  for (int shift = 0;; shift += 7) {
    if (p >= n || shift > 28) return false;
    const uint8_t b = s[p++];
    ulen |= (uint64_t)(b & 0x7f) << shift;
    if (!(b & 0x80)) break;
  }
  out->clear();
  while (p < n) {
    const uint8_t tag = s[p++];
    if ((tag & 3) == 0) {
      size_t len = tag >> 2;
      if (len >= 60) {
        const size_t nb = len - 59;
        if (p + nb > n) return false;
        len = 0;
        for (size_t i = 0; i < nb; ++i) len |= (size_t)s[p + i] << (8 * i);
        p += nb;
      }
      ++len;
      if (p + len > n) return false;
      out->insert(out->end(), s + p, s + p + len);
      p += len;
      continue;
    }
    size_t len, off;
    if ((tag & 3) == 1) {
      if (p + 1 > n) return false;
      len = 4 + (tag >> 2 & 7);
      off = (size_t)(tag >> 5) << 8 | s[p];
      p += 1;
    } else if ((tag & 3) == 2) {
      if (p + 2 > n) return false;
      len = (tag >> 2) + 1;
      off = s[p] | (size_t)s[p + 1] << 8;
      p += 2;
    } else {
      *copy4 = true;
      return false;
    }
    if (off == 0 || off > out->size()) return false;
    if (off > *max_off) *max_off = (uint32_t)off;
    for (size_t i = 0; i < len; ++i) out->push_back((*out)[out->size() - off]);
  }
  return out->size() == ulen;
}

static const uint8_t kGuard = 0xA5;
static const size_t kGuardBytes = 64;

static size_t check_input(const Bytes& in) {
  const size_t n = in.size(), cap = psg_snappy_max_compressed_length(n);
  CHECK(cap == 32 + n + n / 6);
  // exact-length heap buffers on both sides
  uint8_t* src = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(src, in.data(), n);
  uint8_t* dst = (uint8_t*)malloc(cap);
  size_t len = 0;
  CHECK(psg_snappy_compress_host(n ? src : nullptr, n, dst, cap, &len) == PSG_OK);
  CHECK(len >= 1 && len <= cap);
  Bytes back;
  bool copy4 = false;
  uint32_t max_off = 0;
  CHECK(decode(dst, len, &back, &copy4, &max_off));
  CHECK(!copy4 && max_off < 65536);
  CHECK(back == in);
  // the same with a guard behind the maximum length: the same stream, the
  // guard untouched
  uint8_t* wide = (uint8_t*)malloc(cap + kGuardBytes);
  memset(wide, kGuard, cap + kGuardBytes);
  size_t len2 = 0;
  CHECK(psg_snappy_compress_host(src, n, wide, cap, &len2) == PSG_OK);
  CHECK(len2 == len && memcmp(wide, dst, len) == 0);
  for (size_t i = len; i < cap + kGuardBytes; ++i) CHECK(wide[i] == kGuard);
  // one byte of room less is refused and nothing is written
  memset(wide, kGuard, cap);
  size_t len3 = 77;
  CHECK(psg_snappy_compress_host(src, n, wide, cap - 1, &len3) == PSG_ERR_SIZE);
  CHECK(len3 == 77 && wide[0] == kGuard);
  free(wide);
  free(dst);
  free(src);
  return len;
}

int main() {
  // lengths around the literal tag's forms and the 4-byte hash
  for (size_t n : {0, 1, 3, 4, 15, 16, 17, 60, 61}) CHECK(check_input(random_bytes(100 + n, n)) == n + (n > 60 ? 3 : 2) - (n == 0));
  // incompressible runs: 1, 2 and 3 bytes of literal length
  CHECK(check_input(random_bytes(200, 256)) == 256 + 2 + 2);
  CHECK(check_input(random_bytes(201, 257)) == 257 + 2 + 3);
  // (a seed whose 64 KB hold no 4-byte repeat that the table finds)
  CHECK(check_input(random_bytes(204, kFragment)) == kFragment + 3 + 3);
  // fragment seams
  for (size_t n : {kFragment - 1, kFragment, kFragment + 1, 2 * kFragment + 1})
    CHECK(check_input(periodic(n, 7)) < n / 8);
  // the copy-1 / copy-2 seam of the offset
  check_input(repeat(300, 2047, 0, 8));
  check_input(repeat(301, 2048, 0, 8));
  // no match, the minimum, copy-1's limit, one and two copy elements
  for (size_t m : {3, 4, 11, 12, 64, 65}) check_input(repeat(400 + 2 * m, 600, 100, m));
  // the step's seams, and sources that end at and reach into a step's start
  for (size_t n : {kStep - 1, kStep, kStep + 1, 2 * kStep - 1, 2 * kStep, 2 * kStep + 1})
    check_input(periodic(n, 5));
  check_input(repeat(500, 300, kStep - 16, 16));
  check_input(repeat(501, 300, kStep - 15, 16));
  // period 1: every position of a step hits the same table entry
  CHECK(check_input(Bytes(80000, 0)) <= 80000 / 8);
  if (g_bad) {
    printf("test_snappy_enc: %d check(s) failed\n", g_bad);
    return 1;
  }
  printf("test_snappy_enc: ok\n");
  return 0;
}
