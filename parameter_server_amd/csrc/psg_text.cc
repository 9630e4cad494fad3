// psg_text.cc -- the host half of the text ingest: the slow
// tokens through the reference's own libc calls (src/util/strtonum.h), and
// psg_text_parse_host, the same parse done serially into caller arrays.
// Host code only: no HIP call.
#include "psg_text.h"

#include <stdlib.h>
#include <string.h>

#include <string>

#include "psg_host.h"

namespace psg {
namespace text {
namespace {

// strtonum.h:12-32: the value, and whether the whole string was consumed
bool libc_float(const char* s, float* v) {
  char* end;
  *v = strtof(s, &end);
  return *end == '\0';
}
bool libc_i32(const char* s, int32_t* v) {
  char* end;
  *v = (int32_t)strtol(s, &end, 10);
  return *end == '\0';
}
bool libc_u64(const char* s, uint64_t* v) {
  char* end;
  *v = strtoull(s, &end, 10);
  return *end == '\0';
}

// one past the token that starts at s, as strtok_r cuts it; an ADFEA token
// ends with its line
size_t token_end(const unsigned char* t, size_t nbytes, int libsvm, size_t s) {
  size_t e = s;
  while (e < nbytes && !is_delim(libsvm, t[e]))
    if (t[e++] == '\n') break;
  return e;
}

SlowPatch resolve_one(const unsigned char* t, size_t nbytes, int libsvm, bool grouped,
                      const SlowToken& k) {
  SlowPatch p{0, 0.0, 0, 0};
  if (k.start >= nbytes) return p;
  const size_t e = grouped && !libsvm
                       ? k.start + grouped_field(t + k.start, nbytes - k.start, 0xfffffffeu)
                       : token_end(t, nbytes, libsvm, k.start);
  const std::string z((const char*)t + k.start, e - k.start);  // NUL-terminated copy
  switch (k.kind) {
    case kLibsvmLabel: {
      float f;
      p.ok = libc_float(z.c_str(), &f);
      p.val = (double)f;
      break;
    }
    case kLibsvmPair: {
      const size_t c = z.find(':');
      if (c == std::string::npos) break;
      float f = 0;
      p.ok = libc_u64(z.substr(0, c).c_str(), &p.key) && libc_float(z.c_str() + c + 1, &f);
      p.val = (double)f;
      break;
    }
    case kAdfeaLabel: {
      int32_t l;
      p.ok = libc_i32(z.c_str(), &l);
      p.val = l > 0 ? 1.0 : -1.0;
      break;
    }
    case kAdfeaKey:
      p.ok = libc_u64(z.c_str(), &p.key);
      break;
    case kAdfeaSlot: {  // strtoi32, then the ids this library takes (include/psg.h)
      int32_t id;
      p.ok = libc_i32(z.c_str(), &id) && id >= 1 && id < kSlotMax;
      p.key = (uint64_t)(uint32_t)id;
      break;
    }
    default:
      break;
  }
  return p;
}

struct Out {  // the caller's arrays (null: count only) and their room
  uint64_t* offset;
  uint64_t* index;
  double* value;
  double* y;
  uint16_t* slot;  // the grouped parse
  size_t rows_cap, nnz_cap;
};

// One line [ls, le) into row `row`, entries from `*nnz` on.  false: rejected.
// grouped: FileLineReader's chop first, and the ADFEA slot tokens are read.
bool parse_line(const unsigned char* t, size_t nbytes, int libsvm, bool grouped, size_t ls,
                size_t le, const Out& o, size_t row, uint64_t* nnz, uint64_t* slow) {
  if (le - ls >= kMaxLine - 1) return false;
  if (memchr(t + ls, 0, le - ls)) return false;
  const bool ga = grouped && !libsvm;
  if (ga) le = chopped_end(t, ls, le);  // no byte past the chopped line is a token's
  uint32_t ord = 0;
  uint64_t last = 0, key = 0;
  uint16_t slot = 1;
  size_t p = ls;
  for (;; ++ord) {
    while (p < le && is_delim(libsvm, t[p])) ++p;
    if (p >= le) break;
    const size_t e = token_end(t, le, libsvm, p);
    SlowToken st{(uint32_t)p, (uint32_t)row, kNoDest, 0};
    SlowPatch pt{0, 0.0, 1, 0};
    int verdict = kFast;
    if (libsvm) {
      float f = 0;
      if (ord == 0) {
        verdict = libsvm_label(t + p, nbytes - p, &f);
        st.kind = kLibsvmLabel;
      } else {
        verdict = libsvm_pair(t + p, nbytes - p, &pt.key, &f);
        st.kind = kLibsvmPair;
      }
      pt.val = (double)f;
    } else if (ord == 2) {
      verdict = ga ? grouped_label(t + p, nbytes - p, &pt.val)
                   : adfea_label(t + p, nbytes - p, &pt.val);
      st.kind = kAdfeaLabel;
    } else if (ord >= 3 && ord % 2 == 1) {
      verdict = ga ? grouped_key(t + p, nbytes - p, &pt.key)
                   : adfea_key(t + p, nbytes - p, &pt.key);
      st.kind = kAdfeaKey;
    } else if (ga && ord >= 4) {
      uint32_t id = 0;
      verdict = grouped_slot(t + p, nbytes - p, &id);
      if (verdict == kFast && (id < 1 || id >= kSlotMax)) return false;
      slot = (uint16_t)id;
      st.kind = kAdfeaSlot;
    }
    if (verdict == kReject) return false;
    if (verdict == kSlow) {
      ++*slow;
      pt = resolve_one(t, ga ? nbytes : le, libsvm, grouped, st);
      if (!pt.ok) return false;
      if (st.kind == kAdfeaSlot) slot = (uint16_t)pt.key;
    }
    if (libsvm) {
      if (ord == 0) {
        if (o.y && row < o.rows_cap) o.y[row] = pt.val;
      } else {
        if (last > pt.key) return false;  // example_parser.cc:113
        last = pt.key;
        if (o.index && *nnz < o.nnz_cap) o.index[*nnz] = pt.key;
        if (o.value && *nnz < o.nnz_cap) o.value[*nnz] = pt.val;
        if (o.slot && *nnz < o.nnz_cap) o.slot[*nnz] = 1;
        ++*nnz;
      }
    } else if (ord == 2) {
      if (o.y && row < o.rows_cap) o.y[row] = pt.val;
    } else if (ord >= 3 && ord % 2 == 1) {
      key = pt.key;
    } else if (ord >= 4) {
      if (o.index && *nnz < o.nnz_cap) o.index[*nnz] = key;
      if (o.slot && *nnz < o.nnz_cap) o.slot[*nnz] = slot;
      ++*nnz;
    }
    p = e;
  }
  return libsvm ? ord >= 1 : ord >= 3;
}

int parse(const unsigned char* t, size_t nbytes, int libsvm, bool grouped, size_t max_rows,
          bool final, const Out& o, psg_text_result* r) {
  uint64_t rows = 0, nnz = 0, slow = 0;
  size_t at = 0;
  int64_t bad = -1;
  if (o.offset) o.offset[0] = 0;
  while (rows < max_rows && at < nbytes) {
    const unsigned char* nl = (const unsigned char*)memchr(t + at, '\n', nbytes - at);
    if (!nl && !final) break;
    const size_t le = nl ? (size_t)(nl - t) + 1 : nbytes;
    uint64_t n = nnz;
    const bool ok = parse_line(t, nbytes, libsvm, grouped, at, le, o, (size_t)rows, &n, &slow);
    at = le;
    if (!ok) {
      bad = (int64_t)rows;
      break;
    }
    nnz = n;
    ++rows;
    if (o.offset && rows <= o.rows_cap) o.offset[rows] = nnz;
  }
  r->rows = rows;
  r->nnz = nnz;
  r->consumed = at;
  r->bad_line = bad;
  r->slow_tokens = slow;
  r->parse_ms = -1.0;
  return PSG_OK;
}

}  // namespace

void resolve_slow(const unsigned char* text, size_t nbytes, int format_libsvm, int grouped,
                  const SlowToken* tok, size_t n, SlowPatch* patch) {
  for (size_t i = 0; i < n; ++i)
    patch[i] = resolve_one(text, nbytes, format_libsvm, grouped != 0, tok[i]);
}

}  // namespace text
}  // namespace psg

namespace {

int parse_entry(const char* text, size_t nbytes, int format, bool grouped, size_t max_rows,
                int final, uint64_t* offset, uint64_t* index, double* value, double* y,
                uint16_t* slot, size_t rows_cap, size_t nnz_cap, psg_text_result* result) {
  using namespace psg::text;
  if (!result || (nbytes && !text)) return psg::fail(PSG_ERR_ARG, "null argument");
  if (format != PSG_TEXT_ADFEA && format != PSG_TEXT_LIBSVM)
    return psg::fail(PSG_ERR_ARG, "text format %d", format);
  const int libsvm = format == PSG_TEXT_LIBSVM;
  const unsigned char* t = (const unsigned char*)text;
  if ((offset && !y && rows_cap) || (offset && !index && nnz_cap) ||
      (offset && grouped && !slot && nnz_cap))
    return psg::fail(PSG_ERR_ARG, "null output");
  const Out o{offset, offset ? index : nullptr, offset && libsvm ? value : nullptr,
              offset ? y : nullptr, offset && grouped ? slot : nullptr, rows_cap, nnz_cap};
  if (int rc = parse(t, nbytes, libsvm, grouped, max_rows, final != 0, o, result)) return rc;
  if (offset && (result->rows > rows_cap || result->nnz > nnz_cap))
    return psg::fail(PSG_ERR_SIZE, "%llu rows and %llu entries, room for %zu and %zu",
                     (unsigned long long)result->rows, (unsigned long long)result->nnz, rows_cap,
                     nnz_cap);
  return PSG_OK;
}

}  // namespace

extern "C" int psg_text_parse_host(const char* text, size_t nbytes, int format, size_t max_rows,
                                   int final, uint64_t* offset, uint64_t* index, double* value,
                                   double* y, size_t rows_cap, size_t nnz_cap,
                                   psg_text_result* result) {
  return parse_entry(text, nbytes, format, false, max_rows, final, offset, index, value, y,
                     nullptr, rows_cap, nnz_cap, result);
}

extern "C" int psg_text_parse_groups_host(const char* text, size_t nbytes, int format,
                                          size_t max_rows, int final, uint64_t* offset,
                                          uint64_t* index, double* value, double* y,
                                          uint16_t* slot, size_t rows_cap, size_t nnz_cap,
                                          psg_text_result* result) {
  return parse_entry(text, nbytes, format, true, max_rows, final, offset, index, value, y, slot,
                     rows_cap, nnz_cap, result);
}
