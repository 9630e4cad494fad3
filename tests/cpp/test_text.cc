// The fast converters of parameter_server_amd/csrc/psg_text.h against libc,
// and psg_text_parse_host on heap buffers of the exact length, as a
// stand-alone host program (tests/test_text_cpp.py builds it with plain g++
// under the address and undefined-behaviour sanitizers).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/psg.h"
#include "../../parameter_server_amd/csrc/psg_host.h"
#include "../../parameter_server_amd/csrc/psg_text.h"

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

using namespace psg::text;

static const unsigned char* U(const std::string& s) { return (const unsigned char*)s.data(); }

static uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// w with k fraction digits, written out: "123.45" for (12345, 2)
static std::string decimal(uint64_t w, int k, bool neg) {
  std::string d = std::to_string(w);
  if (k > 0) {
    if ((int)d.size() <= k) d = std::string(k + 1 - d.size(), '0') + d;
    d.insert(d.size() - k, ".");
  }
  return (neg ? "-" : "") + d;
}

// the fast form is strtof's whenever it claims the token; the verdict is
// "fast" exactly when the trimmed significand and fraction are in range
static void check_float(const std::string& s, int want_fast) {
  float f = 0;
  const bool fast = fast_float(U(s), (uint32_t)s.size(), &f);
  if (want_fast >= 0) CHECK(fast == (want_fast != 0));
  if (fast) {
    char* end;
    const float g = strtof(s.c_str(), &end);
    CHECK(*end == 0 && fbits(f) == fbits(g));
    if (g_bad && g_bad <= 20 && fbits(f) != fbits(g)) printf("  %s\n", s.c_str());
  }
}

static void test_floats() {
  std::mt19937_64 rng(7);
  for (int k = 0; k <= 10; ++k) {
    for (uint64_t w = (1u << 24) - 4096; w <= (1u << 24); ++w)
      check_float(decimal(w, k, w & 1), w % 10 == 0 && k > 0 ? -1 : 1);
    for (int i = 0; i < 20000; ++i) {
      const uint64_t w = rng() % ((1u << 24) + 1);
      check_float(decimal(w, k, i & 1), w % 10 == 0 && k > 0 ? -1 : 1);
    }
    // just past the edge: slow, unless trailing zeros bring it back
    for (uint64_t w = (1u << 24) + 1; w <= (1u << 24) + 40; ++w)
      check_float(decimal(w, k, false), k > 0 && w % 10 == 0 ? 1 : 0);
  }
  check_float(decimal(1, 11, false), 0);             // 11 fraction digits
  check_float("0.50000000000000000000", 1);          // ... that are trailing zeros
  check_float("1.00000000000", 1);
  check_float("0000000000000000000000016777216", 1);  // leading zeros
  check_float("167772160", 0);                       // an integer's zeros are significant
  check_float("-0", 1);
  check_float("-0.000", 1);
  check_float(std::string(63, '0') + "1", 1);        // 64 bytes
  check_float(std::string(64, '0') + "1", 0);        // 65
  for (const char* s : {"", "-", ".", ".5", "5.", "+1", " 1", "1 ", "1e3", "0x1p-2", "nan", "inf",
                        "1.2.3", "--1", "1-", "1,5"})
    check_float(s, 0);
  float f;
  CHECK(fast_float(U("-0"), 2, &f) && fbits(f) == 0x80000000u);
}

static void check_key(const std::string& s, int want_fast) {
  uint64_t v = 0;
  const bool fast = fast_u64(U(s), (uint32_t)s.size(), &v);
  CHECK(fast == (want_fast != 0));
  if (fast) {
    char* end;
    CHECK(v == strtoull(s.c_str(), &end, 10) && *end == 0);
  }
}

static void test_keys() {
  std::mt19937_64 rng(9);
  const unsigned __int128 one = 1;
  for (unsigned __int128 base : {(unsigned __int128)10000000000000000000ull, (one << 64) - 1,
                                 (one << 63), (unsigned __int128)9999999999999999999ull * 10 + 9}) {
    for (int d = -50; d <= 50; ++d) {
      unsigned __int128 x = base + d;
      std::string s;
      while (x) {
        s.insert(s.begin(), (char)('0' + (int)(x % 10)));
        x /= 10;
      }
      check_key(s, s.size() <= 20);
    }
  }
  check_key("99999999999999999999", 1);   // 20 digits, saturates
  check_key("18446744073709551615", 1);
  check_key("18446744073709551616", 1);
  check_key("100000000000000000000", 0);  // 21 digits
  check_key("00000000000000000001", 1);
  check_key("000000000000000000001", 0);
  for (int i = 0; i < 20000; ++i) check_key(std::to_string(rng() >> (rng() % 64)), 1);
  for (const char* s : {"", "+1", "-1", " 1", "1 ", "1x", "0x1", "1\n"}) check_key(s, 0);
}

static void test_labels() {
  for (long base : {0l, 999999999l, -999999999l, 1000000000l, -1000000000l}) {
    for (long d = -3; d <= 3; ++d) {
      const std::string s = std::to_string(base + d);
      double y = 0;
      const bool fast = fast_label(U(s), (uint32_t)s.size(), &y);
      const size_t digits = s.size() - (s[0] == '-');
      CHECK(fast == (digits <= 9));
      if (fast) CHECK(y == ((int32_t)strtol(s.c_str(), nullptr, 10) > 0 ? 1.0 : -1.0));
    }
  }
  double y;
  CHECK(fast_label(U("-0"), 2, &y) && y == -1.0);
  CHECK(fast_label(U("000000001"), 9, &y) && y == 1.0);
  for (const char* s : {"", "-", "+1", " 1", "1x", "0000000001", "1\n"})
    CHECK(!fast_label(U(s), (uint32_t)strlen(s), &y));
}

// psg_text_parse_host on a malloc'd copy of exactly s.size() bytes: a read
// past the text is a sanitizer report
static psg_text_result parse_exact(const std::string& s, int format, int final) {
  char* t = (char*)malloc(s.size() ? s.size() : 1);
  if (s.size()) memcpy(t, s.data(), s.size());
  psg_text_result r;
  CHECK(psg_text_parse_host(s.size() ? t : t, s.size(), format, 1000, final, nullptr, nullptr,
                            nullptr, nullptr, 0, 0, &r) == PSG_OK);
  std::vector<uint64_t> offset(r.rows + 1), index(r.nnz + 1);
  std::vector<double> value(r.nnz + 1), y(r.rows + 1);
  psg_text_result q;
  CHECK(psg_text_parse_host(t, s.size(), format, 1000, final, offset.data(), index.data(),
                            value.data(), y.data(), r.rows, r.nnz, &q) == PSG_OK);
  CHECK(q.rows == r.rows && q.nnz == r.nnz && q.consumed == r.consumed && q.bad_line == r.bad_line);
  CHECK(offset[r.rows] == r.nnz);
  free(t);
  return r;
}

static void test_exact_buffers() {
  const std::string svm = "1 3:0.5 18446744073709551615:1.25\n-1 7:2";
  const std::string adf = "id 1 1 10:3 18446744073709551615:4\nid 1 0 12:5";
  for (int final = 0; final <= 1; ++final) {
    for (size_t n = 0; n <= svm.size(); ++n) (void)parse_exact(svm.substr(0, n), PSG_TEXT_LIBSVM, final);
    for (size_t n = 0; n <= adf.size(); ++n) (void)parse_exact(adf.substr(0, n), PSG_TEXT_ADFEA, final);
  }
  // right after a ':', inside a token, and with no newline
  psg_text_result r = parse_exact("1 3:", PSG_TEXT_LIBSVM, 1);
  CHECK(r.rows == 1 && r.nnz == 1 && r.bad_line == -1 && r.slow_tokens == 1);
  r = parse_exact("1 3:0.", PSG_TEXT_LIBSVM, 1);
  CHECK(r.rows == 1 && r.slow_tokens == 1);
  r = parse_exact("1 3", PSG_TEXT_LIBSVM, 1);
  CHECK(r.rows == 0 && r.bad_line == 0 && r.consumed == 3);
  r = parse_exact("1 3:1", PSG_TEXT_LIBSVM, 0);
  CHECK(r.rows == 0 && r.bad_line == -1 && r.consumed == 0);
  r = parse_exact("a b 1 5:", PSG_TEXT_ADFEA, 1);
  CHECK(r.rows == 1 && r.nnz == 0);
  r = parse_exact("a b 1 5:2", PSG_TEXT_ADFEA, 1);
  CHECK(r.rows == 1 && r.nnz == 1);
  r = parse_exact(std::string("1 ") + std::string(200, '7'), PSG_TEXT_LIBSVM, 1);  // long, no ':'
  CHECK(r.bad_line == 0 && r.slow_tokens == 1);
  r = parse_exact(std::string("a b 1 ") + std::string(200, '7'), PSG_TEXT_ADFEA, 1);
  CHECK(r.rows == 1 && r.nnz == 0 && r.slow_tokens == 1);
}

int main() {
  test_floats();
  test_keys();
  test_labels();
  test_exact_buffers();
  if (g_bad) {
    printf("test_text: %d check(s) failed\n", g_bad);
    return 1;
  }
  printf("test_text: ok\n");
  return 0;
}
