// psg_text.h -- the token grammar of the text ingest: what
// a byte is to each format, and the fast converters.  A converter takes a
// field [p, p + len) and either gives exactly what the reference's libc call
// gives on it (strtoull / strtol / strtof on the NUL-terminated field,
// src/util/strtonum.h) or says "slow": the field then goes to libc itself
// (psg_text.cc).  The same code runs in the kernels (psg_text.hip), in the
// host parse (psg_text.cc) and in tests/cpp/test_text.cc.
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
namespace text {

constexpr uint32_t kMaxField = 64;        // a longer field is slow
constexpr uint32_t kMaxLine = 60 * 1024;  // kMaxLineLength_, stream_reader.h:36
constexpr uint32_t kMaxSignificand = 1u << 24;
constexpr int kMaxFraction = 10;

// slow-token kinds: what the host resolver calls and where the result goes
enum SlowKind : uint32_t {
  kLibsvmLabel = 0,  // strtof -> y[dest]
  kLibsvmPair = 1,   // idx:val, strtoull and strtof -> index[dest], value[dest]
  kAdfeaLabel = 2,   // strtol -> y[dest]
  kAdfeaKey = 3,     // strtoull -> index[dest]
  kAdfeaSlot = 4     // the grouped parse: strtol truncated to int32 -> slot[dest], 1..4095 or rejected
};
constexpr int64_t kSlotMax = 4096;  // kSlotIDmax, example_parser.h: the ids are 1 .. kSlotMax - 1
constexpr uint32_t kNoDest = 0xffffffffu;  // converted for its verdict only

struct SlowToken {  // one token outside the fast grammar
  uint32_t start;   // its first byte
  uint32_t line;
  uint32_t dest;
  uint32_t kind;
};
struct SlowPatch {  // what libc made of it
  uint64_t key;
  double val;
  uint32_t ok;  // 0: the reference rejects the line
  uint32_t pad;
};

PSG_HD bool is_delim(int format_libsvm, unsigned char c) {
  return format_libsvm ? (c == ' ' || c == '\t' || c == '\r' || c == '\n') : (c == ' ' || c == ':');
}

PSG_HD bool is_digit(unsigned char c) { return (unsigned)(c - '0') < 10u; }

// 1..20 decimal digits; a value past 2^64 - 1 saturates, as strtoull does
PSG_HD bool fast_u64(const unsigned char* p, uint32_t len, uint64_t* out) {
  if (len == 0 || len > 20) return false;
  uint64_t v = 0;
  bool over = false;
  for (uint32_t i = 0; i < len; ++i) {
    if (!is_digit(p[i])) return false;
    const uint64_t d = (uint64_t)(p[i] - '0');
    if (v > 1844674407370955161ull || (v == 1844674407370955161ull && d > 5)) over = true;
    v = v * 10u + d;
  }
  *out = over ? ~0ull : v;
  return true;
}

// an optional '-' and 1..9 digits: label > 0 ? 1 : -1 (example_parser.cc:144)
PSG_HD bool fast_label(const unsigned char* p, uint32_t len, double* y) {
  uint32_t i = 0;
  if (len && p[0] == '-') i = 1;
  if (len - i == 0 || len - i > 9) return false;
  uint32_t v = 0;
  for (uint32_t j = i; j < len; ++j) {
    if (!is_digit(p[j])) return false;
    v = v * 10u + (uint32_t)(p[j] - '0');
  }
  *y = (i == 0 && v > 0) ? 1.0 : -1.0;
  return true;
}

// -?digits(.digits)? whose decimal significand w (leading zeros and trailing
// fraction zeros dropped) is at most 2^24 with k <= 10 fraction digits:
// (float)((double)w / 10^k), correctly rounded
PSG_HD bool fast_float(const unsigned char* p, uint32_t len, float* out) {
  if (len == 0 || len > kMaxField) return false;
  uint32_t i = 0;
  const bool neg = p[0] == '-';
  if (neg) i = 1;
  uint32_t int_end = i;
  while (int_end < len && is_digit(p[int_end])) ++int_end;
  if (int_end == i) return false;
  uint32_t end = int_end;  // one past the last significant digit
  if (int_end < len) {
    if (p[int_end] != '.' || int_end + 1 == len) return false;
    for (uint32_t j = int_end + 1; j < len; ++j)
      if (!is_digit(p[j])) return false;
    end = len;
    while (end > int_end + 1 && p[end - 1] == '0') --end;
    if (end == int_end + 1) end = int_end;  // the fraction is all zeros
  }
  const int k = end > int_end ? (int)(end - int_end - 1) : 0;
  if (k > kMaxFraction) return false;
  uint32_t w = 0;
  for (uint32_t j = i; j < end; ++j) {
    if (j == int_end) continue;  // the point
    w = w * 10u + (uint32_t)(p[j] - '0');
    if (w > kMaxSignificand) return false;
  }
  double scale = 1.0;  // 10^k, exact for k <= 22
  for (int j = 0; j < k; ++j) scale = scale * 10.0;
  const float f = (float)((double)w / scale);
  *out = neg ? -f : f;
  return true;
}

// What a token is to the fast grammar.  p: its first byte; avail: the bytes
// from p to the end of the text.  At most 2 * kMaxField + 2 bytes are read.
enum Verdict { kFast = 0, kSlow = 1, kReject = 2 };

// a LIBSVM label: the token is one float field
PSG_HD int libsvm_label(const unsigned char* p, size_t avail, float* label) {
  uint32_t e = 0;
  while (e < avail && e <= kMaxField && !is_delim(1, p[e])) ++e;
  if (e > kMaxField) return kSlow;
  return fast_float(p, e, label) ? kFast : kSlow;
}

// a LIBSVM idx:val token, split at its first ':' (example_parser.cc:106-112);
// without one the line is rejected (:107)
PSG_HD int libsvm_pair(const unsigned char* p, size_t avail, uint64_t* idx, float* val) {
  uint32_t c = 0;
  while (c < avail && c <= kMaxField && p[c] != ':' && !is_delim(1, p[c])) ++c;
  if (c > kMaxField) return kSlow;
  if (c == avail || p[c] != ':') return kReject;
  uint32_t e = c + 1;
  while (e < avail && e - c - 1 <= kMaxField && !is_delim(1, p[e])) ++e;
  if (e - c - 1 > kMaxField) return kSlow;
  return fast_u64(p, c, idx) && fast_float(p + c + 1, e - c - 1, val) ? kFast : kSlow;
}

// the digits of an ADFEA token: a '\n' in it (the line's end) makes it slow,
// and libc then rejects it
PSG_HD uint32_t adfea_field(const unsigned char* p, size_t avail, bool* slow) {
  uint32_t e = 0;
  while (e < avail && e <= kMaxField && !is_delim(0, p[e]) && p[e] != '\n') ++e;
  *slow = e > kMaxField || (e < avail && p[e] == '\n');
  return e;
}
PSG_HD int adfea_label(const unsigned char* p, size_t avail, double* y) {
  bool slow;
  const uint32_t e = adfea_field(p, avail, &slow);
  return !slow && fast_label(p, e, y) ? kFast : kSlow;
}
PSG_HD int adfea_key(const unsigned char* p, size_t avail, uint64_t* key) {
  bool slow;
  const uint32_t e = adfea_field(p, avail, &slow);
  return !slow && fast_u64(p, e, key) ? kFast : kSlow;
}


// ---- the grouped parse (include/psg.h, "Text ingest by feature group") --------
// 1..4 decimal digits: the slot id strtoi32 gives ("07" is 7).  The range
// [1, kSlotMax) is the caller's check.
PSG_HD bool fast_slot(const unsigned char* p, uint32_t len, uint32_t* id) {
  if (len == 0 || len > 4) return false;
  uint32_t v = 0;
  for (uint32_t i = 0; i < len; ++i) {
    if (!is_digit(p[i])) return false;
    v = v * 10u + (uint32_t)(p[i] - '0');
  }
  *id = v;
  return true;
}
// A byte of the grouped ADFEA parse that no token holds: a delimiter, the
// line's '\n', and the one '\r' that FileLineReader chops: directly before
// the '\n', or the last byte of the text (a final line without '\n'; a
// partial line that is not final is not taken at all).  next: the byte after
// c; at_end: there is none.
PSG_HD bool grouped_gap(unsigned char c, unsigned char next, bool at_end) {
  return c == ' ' || c == ':' || c == '\n' || (c == '\r' && (at_end || next == '\n'));
}
// the length of the token at p, up to max + 1; avail: the bytes from p to the
// end of the text
PSG_HD uint32_t grouped_field(const unsigned char* p, size_t avail, uint32_t max) {
  uint32_t e = 0;
  while (e < avail && e <= max &&
         !grouped_gap(p[e], e + 1 < avail ? p[e + 1] : (unsigned char)0, e + 1 == avail))
    ++e;
  return e;
}
// A further token follows, on its line, the token that ends at p: a key whose
// slot token is missing is parsed and dropped (example_parser.cc:146-155).
PSG_HD bool grouped_follows(const unsigned char* p, size_t avail) {
  size_t i = 0;
  while (i < avail && (p[i] == ' ' || p[i] == ':')) ++i;
  return i < avail && !grouped_gap(p[i], i + 1 < avail ? p[i + 1] : (unsigned char)0, i + 1 == avail);
}
PSG_HD int grouped_label(const unsigned char* p, size_t avail, double* y) {
  const uint32_t e = grouped_field(p, avail, kMaxField);
  return e <= kMaxField && fast_label(p, e, y) ? kFast : kSlow;
}
PSG_HD int grouped_key(const unsigned char* p, size_t avail, uint64_t* key) {
  const uint32_t e = grouped_field(p, avail, kMaxField);
  return e <= kMaxField && fast_u64(p, e, key) ? kFast : kSlow;
}
PSG_HD int grouped_slot(const unsigned char* p, size_t avail, uint32_t* id) {
  return fast_slot(p, grouped_field(p, avail, 4), id) ? kFast : kSlow;
}
// FileLineReader's chop (util/filelinereader.cc:37-42): the end of the line
// [ls, le) once its '\n' and then at most one '\r' are gone
PSG_HD size_t chopped_end(const unsigned char* t, size_t ls, size_t le) {
  if (le > ls && t[le - 1] == '\n') --le;
  if (le > ls && t[le - 1] == '\r') --le;
  return le;
}

// The slow tokens through libc (psg_text.cc; host only).  patch[i] is what
// the reference's call makes of tok[i].
// grouped: the tokens are cut by the grouped parse's line rule.
void resolve_slow(const unsigned char* text, size_t nbytes, int format_libsvm, int grouped,
                  const SlowToken* tok, size_t n, SlowPatch* patch);

}  // namespace text
}  // namespace psg
