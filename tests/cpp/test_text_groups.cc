// The grouped host parse (psg_text_parse_groups_host, psg_text.cc) and its
// shared pieces (psg_text.h: fast_slot, grouped_slot, chopped_end) on heap
// buffers of the exact length, as a stand-alone host program
// (tests/test_text_groups_cpp.py builds it with plain g++ under the address
// and undefined-behaviour sanitizers): a read past the text, or past an
// output array of exactly the reported size, is a sanitizer report.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static void test_slot_converters() {
  for (int v = 0; v <= 10000; v += (v < 20 ? 1 : 37)) {
    const std::string s = std::to_string(v);
    uint32_t id = 77777;
    const bool fast = fast_slot(U(s), (uint32_t)s.size(), &id);
    CHECK(fast == (s.size() <= 4));
    if (fast) CHECK(id == (uint32_t)v);
  }
  uint32_t id = 0;
  CHECK(fast_slot(U("07"), 2, &id) && id == 7);
  CHECK(fast_slot(U("0007"), 4, &id) && id == 7);
  CHECK(!fast_slot(U("00007"), 5, &id));
  CHECK(!fast_slot(U("+7"), 2, &id));
  CHECK(!fast_slot(U(""), 0, &id));
  CHECK(!fast_slot(U("7\r"), 2, &id));
  // grouped_slot reads at most six bytes and never past `avail`
  for (const std::string& s : {std::string("7"), std::string("4095"), std::string("40950"),
                               std::string("12 3"), std::string("1:2"), std::string("7\r"),
                               std::string("7\r\n"), std::string("7\r\r\n"), std::string("7\n")}) {
    unsigned char* t = (unsigned char*)malloc(s.size());
    memcpy(t, s.data(), s.size());
    const int v = grouped_slot(t, s.size(), &id);
    CHECK(v == (s == "40950" || s == "7\r\r\n" ? kSlow : kFast));
    free(t);
  }
  const std::string l = "ab\r\r\n";
  CHECK(chopped_end(U(l), 0, 5) == 3);
  CHECK(chopped_end(U(l), 0, 4) == 3);  // a final line ending in '\r'
  CHECK(chopped_end(U(l), 0, 2) == 2);
  CHECK(chopped_end(U(l), 4, 5) == 4);  // "\n" alone
  CHECK(chopped_end(U(l), 3, 5) == 3);  // "\r\n" alone
  CHECK(chopped_end(U(l), 2, 2) == 2);  // an empty line
}

struct Parsed {
  psg_text_result r;
  std::vector<uint64_t> offset, index;
  std::vector<double> value, y;
  std::vector<uint16_t> slot;
};

// on a malloc'd copy of exactly s.size() bytes, into arrays of exactly the
// sizes the first call reports
static Parsed parse_exact(const std::string& s, int format, int final, size_t max_rows = 1000) {
  char* t = (char*)malloc(s.size() ? s.size() : 1);
  memcpy(t, s.data(), s.size());
  Parsed p;
  CHECK(psg_text_parse_groups_host(t, s.size(), format, max_rows, final, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, 0, 0, &p.r) == PSG_OK);
  uint64_t* offset = (uint64_t*)malloc(8 * (p.r.rows + 1));
  uint64_t* index = (uint64_t*)malloc(p.r.nnz ? 8 * p.r.nnz : 1);
  double* value = (double*)malloc(p.r.nnz ? 8 * p.r.nnz : 1);
  double* y = (double*)malloc(p.r.rows ? 8 * p.r.rows : 1);
  uint16_t* slot = (uint16_t*)malloc(p.r.nnz ? 2 * p.r.nnz : 1);
  psg_text_result q;
  CHECK(psg_text_parse_groups_host(t, s.size(), format, max_rows, final, offset, index, value, y,
                                   slot, p.r.rows, p.r.nnz, &q) == PSG_OK);
  CHECK(q.rows == p.r.rows && q.nnz == p.r.nnz && q.consumed == p.r.consumed &&
        q.bad_line == p.r.bad_line && q.slow_tokens == p.r.slow_tokens);
  CHECK(offset[p.r.rows] == p.r.nnz);
  p.offset.assign(offset, offset + p.r.rows + 1);
  p.index.assign(index, index + p.r.nnz);
  if (format == PSG_TEXT_LIBSVM) p.value.assign(value, value + p.r.nnz);
  p.y.assign(y, y + p.r.rows);
  p.slot.assign(slot, slot + p.r.nnz);
  free(t);
  free(offset);
  free(index);
  free(value);
  free(y);
  free(slot);
  return p;
}

static void test_exact_buffers() {
  {  // every rule's line as the last bytes of the buffer
    const Parsed p = parse_exact("a 1 1 5:2 9:4095\r\nb 1 0 7:00007 8", PSG_TEXT_ADFEA, 1);
    CHECK(p.r.rows == 2 && p.r.nnz == 3 && p.r.bad_line == -1 && p.r.slow_tokens == 1);
    CHECK(p.slot == (std::vector<uint16_t>{2, 4095, 7}));
    CHECK(p.index == (std::vector<uint64_t>{5, 9, 7}));
    CHECK(p.offset == (std::vector<uint64_t>{0, 2, 3}));
    CHECK(p.y == (std::vector<double>{1.0, -1.0}));
  }
  {
    const Parsed p = parse_exact("a 1 1 5:2 9:4095\r\nb 1 0 7:00007 8", PSG_TEXT_ADFEA, 0);
    CHECK(p.r.rows == 1 && p.r.nnz == 2 && p.r.consumed == 18);
  }
  for (const char* tail : {"7", "7\r", "4095", "4096", "0", "-1", "+7", "\t7", "4294967297", "7x",
                           "77777", "", "\r", "\r\r", ":", " "}) {
    for (const char* nl : {"", "\n", "\r\n"}) {
      const std::string s = std::string("a 1 1 5:1\nb 1 1 6:") + tail + nl;
      for (int final = 0; final <= 1; ++final) {
        const Parsed p = parse_exact(s, PSG_TEXT_ADFEA, final);
        CHECK(p.r.rows >= 1 && p.r.rows <= 2);
        CHECK(p.r.consumed <= s.size());
        for (uint16_t id : p.slot) CHECK(id >= 1 && id < 4096);
      }
    }
  }
  {  // a key, a label and a slot each ending the buffer with no byte after
    CHECK(parse_exact("a 1 1", PSG_TEXT_ADFEA, 1).r.rows == 1);
    CHECK(parse_exact("a 1 1 18446744073709551615", PSG_TEXT_ADFEA, 1).r.nnz == 0);
    CHECK(parse_exact("a 1 1 18446744073709551615:4095", PSG_TEXT_ADFEA, 1).r.nnz == 1);
    CHECK(parse_exact("a 1", PSG_TEXT_ADFEA, 1).r.bad_line == 0);
    CHECK(parse_exact("\r", PSG_TEXT_ADFEA, 1).r.bad_line == 0);
    CHECK(parse_exact("", PSG_TEXT_ADFEA, 1).r.rows == 0);
  }
  {
    const Parsed p = parse_exact("1 3:0.5 18446744073709551615:1.25\r\n-1 7:2", PSG_TEXT_LIBSVM, 1);
    CHECK(p.r.rows == 2 && p.r.nnz == 3);
    CHECK(p.slot == (std::vector<uint16_t>{1, 1, 1}));
    CHECK(p.value == (std::vector<double>{0.5, 1.25, 2.0}));
  }
  {  // max_rows stops before a rejected line
    const Parsed p = parse_exact("a 1 1 5:1\nb 1 1 5:0\n", PSG_TEXT_ADFEA, 1, 1);
    CHECK(p.r.rows == 1 && p.r.bad_line == -1 && p.r.consumed == 10);
  }
  {  // a line of the length limit: '\r' and '\n' are counted
    std::string s = "a 1 1";
    while (s.size() < kMaxLine - 4) s += " 5:1";
    s.resize(kMaxLine - 4);  // ... then "\r\n": kMaxLine - 2 bytes, the longest line taken
    CHECK(parse_exact(s + "\r\n", PSG_TEXT_ADFEA, 1).r.bad_line == -1);
    CHECK(parse_exact(s + " \r\n", PSG_TEXT_ADFEA, 1).r.bad_line == 0);
  }
}

int main() {
  test_slot_converters();
  test_exact_buffers();
  if (g_bad) {
    printf("%d checks failed\n", g_bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
