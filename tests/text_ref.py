"""The text reader of the reference restated in Python, for the text ingest
tests: StreamReader::readMatricesFromText (src/data/stream_reader.h:50-122)
over ExampleParser::parseLibsvm / parseAdfea (src/data/example_parser.cc:84-160)
with ignore_feature_group = true.  Lines are cut by fgets' rule, tokens as
strtok_r cuts them, and every number goes through libc's own strtof /
strtoull / strtol (src/util/strtonum.h) by ctypes.  The defined deviations of
include/psg.h (each a rejected line) are restated too.  Unpinned: the
reference's parser itself is not compiled in."""
import ctypes
import re

import numpy as np

ADFEA, LIBSVM = 4, 5
MAX_LINE = 60 * 1024  # kMaxLineLength_
MAX_FIELD = 64

_libc = ctypes.CDLL(None)
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
_libc.strtoull.restype = ctypes.c_ulonglong
_libc.strtoull.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
_libc.strtol.restype = ctypes.c_long
_libc.strtol.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]


def _conv(fn, tok, *extra):
    """fn(tok) and whether it consumed the string (*end == 0)."""
    buf = ctypes.create_string_buffer(tok)
    end = ctypes.c_void_p()
    v = fn(buf, ctypes.byref(end), *extra)
    k = end.value - ctypes.addressof(buf)
    return v, buf.raw[k] == 0


def strtofloat(tok):
    return _conv(_libc.strtof, tok)


def strtou64(tok):
    return _conv(_libc.strtoull, tok, 10)


def strtoi32(tok):
    v, ok = _conv(_libc.strtol, tok, 10)
    v &= 0xFFFFFFFF  # *num = strtol(...) into an int32
    return (v - (1 << 32) if v >= 1 << 31 else v), ok


def lines_of(text, final):
    """fgets: bytes up to and including '\\n'; the rest counts when final."""
    out, at = [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        if nl < 0:
            if final:
                out.append(text[at:])
            break
        out.append(text[at:nl + 1])
        at = nl + 1
    return out


def tokens_of(line, fmt):
    """strtok_r: maximal runs of bytes outside the delimiter set."""
    return [t for t in re.split(rb"[ \t\r\n]+" if fmt == LIBSVM else rb"[ :]+", line) if t]


def parse_line(line, fmt):
    """(y, keys, vals) or None: the line is rejected."""
    if len(line) >= MAX_LINE - 1 or b"\0" in line:
        return None
    tok = tokens_of(line, fmt)
    keys, vals = [], []
    if fmt == LIBSVM:
        if not tok:
            return None
        label, ok = strtofloat(tok[0])
        if not ok:
            return None
        last = 0
        for t in tok[1:]:
            c = t.find(b":")
            if c < 0:
                return None
            idx, ok1 = strtou64(t[:c])
            if not ok1:
                return None
            val, ok2 = strtofloat(t[c + 1:])
            if not ok2 or last > idx:
                return None
            last = idx
            keys.append(idx)
            vals.append(val)
        return float(label), keys, vals
    if len(tok) < 3:
        return None
    label, ok = strtoi32(tok[2])
    if not ok:
        return None
    key = None
    for i, t in enumerate(tok[3:], 3):
        if i % 2 == 1:
            key, ok = strtou64(t)
            if not ok:
                return None
        else:
            keys.append(key)
    return (1.0 if label > 0 else -1.0), keys, None


def parse(text, fmt, max_rows=None, final=True):
    """(offset, index, value or None, y, rows, consumed, bad_line)."""
    offset, index, value, y = [0], [], [], []
    consumed, bad = 0, -1
    for line in lines_of(text, final):
        if max_rows is not None and len(y) >= max_rows:
            break
        consumed += len(line)
        r = parse_line(line, fmt)
        if r is None:
            bad = len(y)
            break
        y.append(r[0])
        index.extend(r[1])
        if fmt == LIBSVM:
            value.extend(r[2])
        offset.append(len(index))
    val = np.array(value, dtype=np.float32).astype(np.float64) if fmt == LIBSVM else None
    return (np.array(offset, dtype=np.uint64), np.array(index, dtype=np.uint64), val,
            np.array(y, dtype=np.float64), len(y), consumed, bad)


# ---- the fast grammar of include/psg.h, by regular expressions ---------------
def fast_key(t):
    return re.fullmatch(rb"[0-9]{1,20}", t) is not None


def fast_label(t):
    return re.fullmatch(rb"-?[0-9]{1,9}", t) is not None


def fast_float(t):
    m = re.fullmatch(rb"-?([0-9]+)(?:\.([0-9]+))?", t)
    if m is None or len(t) > MAX_FIELD:
        return False
    frac = (m.group(2) or b"").rstrip(b"0")
    return int(m.group(1) + frac) <= 1 << 24 and len(frac) <= 10


def slow_tokens(text, fmt, max_rows=None, final=True, stop_at_bad=False):
    """Tokens outside the fast grammar among the lines taken; with
    stop_at_bad, up to the token that rejects a line (psg_text_parse_host)."""
    n = 0
    for row, line in enumerate(lines_of(text, final)):
        if max_rows is not None and row >= max_rows:
            break
        if stop_at_bad and (len(line) >= MAX_LINE - 1 or b"\0" in line):
            break
        bad = parse_line(line, fmt) is None
        last = 0
        for i, t in enumerate(tokens_of(line, fmt)):
            slow, stop = False, False
            if fmt == LIBSVM:
                if i == 0:
                    slow = len(t) > MAX_FIELD or not fast_float(t)
                    stop = not strtofloat(t)[1]
                else:
                    c = t[:MAX_FIELD + 1].find(b":")
                    if c < 0:
                        slow = len(t) > MAX_FIELD  # a short token without ':' is rejected on sight
                    else:
                        slow = (len(t) - c - 1 > MAX_FIELD or not fast_key(t[:c])
                                or not fast_float(t[c + 1:]))
                    one = parse_line(b"0 " + t, fmt)
                    stop = one is None or last > one[1][0]
                    last = one[1][0] if one else last
            elif i == 2:
                slow = len(t) > MAX_FIELD or not fast_label(t)
                stop = not strtoi32(t)[1]
            elif i >= 3 and i % 2 == 1:
                slow = len(t) > MAX_FIELD or not fast_key(t)
                stop = not strtou64(t)[1]
            n += 1 if slow else 0
            if stop_at_bad and stop:
                break
        if stop_at_bad and bad:
            break
    return n
