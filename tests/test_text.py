"""CPU: the text ingest's host parse (psg_text_parse_host,
parameter_server_amd/csrc/psg_text.cc) against the restatement of the
reference's reader (tests/text_ref.py), bit for bit, and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import text_ref as T
from parameter_server_amd import _lib
from parameter_server_amd.worker import parse_text_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (T.LIBSVM, T.ADFEA)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(text, fmt, max_rows=None, final=True):
    """psg_text_parse_host == the restatement; returns the result struct."""
    offset, index, value, y, rows, consumed, bad = T.parse(text, fmt, max_rows, final)
    o, i, v, yy, r = parse_text_host(text, fmt, max_rows, final)
    what = (text[:80], fmt, max_rows, final)
    assert (r.rows, r.nnz, r.consumed, r.bad_line) == (rows, index.size, consumed, bad), what
    assert np.array_equal(o, offset), what
    assert np.array_equal(i, index), what
    assert np.array_equal(bits(yy), bits(y)), what
    if fmt == T.LIBSVM:
        assert np.array_equal(bits(v), bits(value)), what
    else:
        assert v is None
    assert r.slow_tokens == T.slow_tokens(text, fmt, max_rows, final, stop_at_bad=True), what
    assert r.parse_ms == -1.0
    return r


# ---- a seeded corpus ------------------------------------------------------------
def corpus(fmt, lines=3000, seed=11):
    """Lines of either format with mostly fast tokens and a sprinkle of every
    slow kind; no rejected line."""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(lines):
        nf = int(rng.integers(0, 12))
        if fmt == T.ADFEA:
            nf = max(nf, 1)  # an ADFEA line ends in a slot token, or it is rejected
        keys = np.sort(rng.integers(0, 1 << 63, nf, dtype=np.uint64) * 2 + rng.integers(0, 2))
        if fmt == T.LIBSVM:
            lab = ("%d" % rng.integers(-1, 2)) if r % 7 else "%.3f" % rng.normal()
            parts = [lab]
            for k in keys:
                kind = int(rng.integers(0, 10))
                if kind == 0:
                    val = "%.3e" % rng.normal()
                elif kind == 1:
                    val = "%d" % rng.integers(-(1 << 25), 1 << 25)
                elif kind == 2:
                    val = "%.12f" % rng.normal()
                else:
                    val = "%.6f" % rng.normal()
                parts.append("%d:%s" % (int(k), val))
            sep = "\t" if r % 5 == 0 else " "
            out.append(sep.join(parts) + ("\r\n" if r % 3 == 0 else "\n"))
        else:
            lab = "%d" % rng.integers(-2, 3)
            if r % 11 == 0:
                lab = "+1"
            parts = ["%d 1 %s" % (r, lab)]
            for k in keys:
                key = "%d" % int(k) if rng.integers(0, 9) else "+%d" % int(k)
                parts.append("%s:%d" % (key, rng.integers(0, 100)))
            out.append(" ".join(parts) + ("\r\n" if r % 3 == 0 else "\n"))
    return "".join(out).encode()


@pytest.mark.parametrize("fmt", FORMATS)
def test_corpus(fmt):
    text = corpus(fmt)
    r = check(text, fmt)
    assert r.bad_line == -1 and r.rows == 3000 and r.consumed == len(text)
    assert 0 < r.slow_tokens
    check(text, fmt, max_rows=1234)
    check(text[:-1], fmt, final=False)
    check(text[:-1], fmt, final=True)


# ---- every quirk and deviation, one line each -------------------------------------
K64 = (1 << 64) - 1
LIBSVM_LINES = [
    b"1 3:0.5 7:1\n",
    b"-1 3:0.5 7:1\r\n",                      # CRLF
    b"  \t 1 \t\t 3:2   9:4 \t\n",            # runs of blanks and tabs
    b"0.25\n",                                  # label only
    b"1 :5\n", b"1 3:\n", b"1 +7:1\n", b"1 7:+1\n", b"1 3:1e-3\n", b"1 3:0x1p-2\n",
    b"nan 1:nan\n", b"inf 2:-inf\n", b"1 3:.5\n", b"1 3:5.\n", b"+1\n", b"1e0\n",
    b"1 %d:1\n" % K64, b"1 %d:1\n" % (K64 + 1), b"1 %d:1\n" % (10 ** 19), b"1 %s:1\n" % (b"9" * 25),
    b"1 00000000000000000000123:1\n",
    b"-0 1:-0 2:-0.0 3:-0.000\n",
    b"1 1:16777216 2:16777217 3:99999999 4:123456789 5:1.6777216 6:0.16777217\n",  # 8, 9 digits
    b"1 1:0.0000000001 2:0.00000000001 3:0.12345678901 4:1.50000000000000\n",      # 10, 11 places
    b"1 1:000000000000000000000000000000000000000000000000000000000000001.5\n",  # 65 bytes
    b"1 1:00000000000000000000000000000000000000000000000000000000000001.5\n",   # 64 bytes
    b"1 5:1 5:2 6:3\n",                         # equal idx
    b"1 5:1 4:2\n",                             # descending: rejected
    b"1 9:1\n",
    b"1 3\n",                                   # no ':': rejected
    b"1 3:1:2\n",                               # strtof stops at ':': rejected
    b"1x 3:1\n", b"1 3x:1\n", b"1 3:1x\n", b"1 -3:1\n", b"1 3 :1\n",
    b"\n",                                      # no token: rejected
    b" \t\r\n",
    b"1 1:1\0 2:2\n",                           # NUL: rejected
    b"1 " + b"7:1 " * 15400 + b"\n",            # 61603 bytes: rejected
    b"1 " + b"1:2 " * 15358 + b"1:2345\n",      # 61441 bytes
    b"1 " + b" " * 61435 + b"\n",               # 61438 bytes: the longest line taken
    b"1  " + b" " * 61435 + b"\n",              # 61439 bytes: rejected
    b"1 " + b"8" * 70 + b":1\n", b"1 " + b"8" * 70 + b"\n", b"1 1:" + b"1" * 70 + b"\n",
    b"1 3:2",                                   # no trailing newline
]
ADFEA_LINES = [
    b"id 1 1 10:1 20:2\n",
    b"id 1 0 10:1 20:2\r\n",                    # the slot token carries "\r\n"
    b"id 1 -1 10:1\n",
    b"id 1 1 10:1 20:2 \n",                     # "\n" is a key token: rejected
    b"id 1 1\n",                                # the label ends in '\n': rejected
    b"id 1 1 10\n",                             # a key ends in '\n': rejected
    b"id 1 1 \n",                               # "\n" as a key: rejected
    b"id 1\n", b"id\n", b"\n", b" : \n",      # fewer than three tokens: rejected
    b"id::1 : 1 ::10 :: 1\n",                   # runs of delimiters
    b"id\t1 1 10:1\n",                          # a tab is a token byte: "id\t1" "1" "10" ...
    b"a b 5 10:x 20:\ty 30:1\n",                # slot ids are not parsed
    b"a b 999999999 1:1\n", b"a b -999999999 1:1\n", b"a b 1000000000 1:1\n",
    b"a b 2147483648 1:1\n", b"a b 4294967297 1:1\n", b"a b -4294967295 1:1\n",
    b"a b 99999999999999999999 1:1\n", b"a b +1 1:1\n", b"a b  1 1:1\n", b"a b 1x 1:1\n",
    b"a b -0 1:1\n", b"a b - 1:1\n",
    b"a b 1 %d:1 %d:1 %d:1 %s:1\n" % (K64, K64 + 1, 10 ** 19, b"9" * 25),
    b"a b 1 +7:1 -7:1\n", b"a b 1 7x:1\n", b"a b 1 0x7:1\n", b"a b 1 \t7:1\n",
    b"a b 1 1:1\0 2:2\n",                       # NUL: rejected
    b"a b 1 " + b"7:1 " * 15400 + b"\n",        # too long: rejected
    b"a b 1 " + b"1" * 70 + b":1\n",
    b"a b 1 10:1 20",                           # final line: the key without a slot is dropped
    b"a b 1 10:1 20x",                          # ... but parsed: rejected
    b"a b 1",                                   # label at the end of the text
    b"a b 1 10:1",
]


@pytest.mark.parametrize("fmt", FORMATS)
def test_quirk_lines(fmt):
    lines = LIBSVM_LINES if fmt == T.LIBSVM else ADFEA_LINES
    rejected = 0
    for line in lines:
        for final in (True, False):
            r = check(line, fmt, final=final)
            rejected += r.bad_line == 0
            if not line.endswith(b"\n") and not final:
                assert (r.rows, r.consumed, r.bad_line) == (0, 0, -1)
    assert rejected >= 10


@pytest.mark.parametrize("fmt", FORMATS)
def test_rejected_line_first_middle_last(fmt):
    good = b"1 3:1 4:2\n" if fmt == T.LIBSVM else b"a b 1 3:1 4:2\n"
    bad = b"1 4:1 3:2\n" if fmt == T.LIBSVM else b"a b 1 3:1 4\n"
    for text, at in ((bad + good * 3, 0), (good * 2 + bad + good, 2), (good * 3 + bad, 3)):
        r = check(text, fmt)
        assert (r.rows, r.bad_line, r.consumed) == (at, at, len(good) * at + len(bad))
        # the caller walks on past the rejected line
        rest = check(text[r.consumed:], fmt)
        assert rest.rows == 3 - at and rest.bad_line == -1
        assert check(text, fmt, max_rows=at).bad_line == -1  # not reached


@pytest.mark.parametrize("fmt", FORMATS)
def test_max_rows_final_and_empty(fmt):
    good = b"1 3:1 4:2\n" if fmt == T.LIBSVM else b"a b 1 3:1 4:2\n"
    for final in (True, False):
        assert check(b"", fmt, final=final).consumed == 0
        for cap in (0, 1, 2, 5, 6, None):
            check(good * 5, fmt, cap, final)
            check(good * 5 + good[:-1], fmt, cap, final)
    assert check(good * 5 + good[:-1], fmt, final=True).rows == 6
    assert check(good * 5 + good[:-1], fmt, final=False).rows == 5


def test_quirks_as_one_walk():
    """The quirk lists as one text each, walked by `consumed` to the end."""
    for fmt, lines in ((T.LIBSVM, LIBSVM_LINES), (T.ADFEA, ADFEA_LINES)):
        text = b"".join(l if l.endswith(b"\n") else l + b"\n" for l in lines)
        at, loads = 0, 0
        while at < len(text):
            r = check(text[at:], fmt)
            assert r.consumed > 0
            at += r.consumed
            loads += 1
        assert loads > 10


# ---- the ABI ------------------------------------------------------------------------
def test_abi_names():
    src = open(os.path.join(ROOT, "include", "psg.h")).read()
    for name in ("psg_mb_load_text", "psg_text_parse_host", "psg_text_chunk"):
        assert re.search(r"\b%s\(" % name, src) and name in _lib.SIGNATURES
    assert "#define PSG_ABI_VERSION 1" in src
    L = _lib.lib()
    assert L.psg_abi_version() == 1
    c = L.psg_text_chunk()
    assert c >= 256 and c % 16 == 0
    assert (_lib.PSG_TEXT_ADFEA, _lib.PSG_TEXT_LIBSVM) == (4, 5)
    for name, val in (("PSG_TEXT_ADFEA", 4), ("PSG_TEXT_LIBSVM", 5), ("PSG_MB_OFFSET", 24),
                      ("PSG_MB_INDEX", 25), ("PSG_MB_VALUE", 26), ("PSG_MB_Y", 27)):
        assert re.search(r"#define %s %d\b" % (name, val), src) and getattr(_lib, name) == val


def test_abi_bad_arguments():
    L = _lib.lib()
    r = _lib.TextResult()
    t = b"1 1:1\n"
    ok = lambda *a: L.psg_text_parse_host(*a)
    assert ok(t, len(t), 5, 10, 1, None, None, None, None, 0, 0, C.byref(r)) == _lib.PSG_OK
    assert (r.rows, r.nnz) == (1, 1)
    assert ok(t, len(t), 5, 10, 1, None, None, None, None, 0, 0, None) == _lib.PSG_ERR_ARG
    assert ok(None, len(t), 5, 10, 1, None, None, None, None, 0, 0, C.byref(r)) == _lib.PSG_ERR_ARG
    for fmt in (0, 3, 6, -1):  # TERAFEA (6 in DataConfig is not ours) and nonsense
        assert ok(t, len(t), fmt, 10, 1, None, None, None, None, 0, 0,
                  C.byref(r)) == _lib.PSG_ERR_ARG
        assert L.psg_mb_load_text(None, t, len(t), fmt, 10, 1, C.byref(r)) == _lib.PSG_ERR_ARG
    assert L.psg_mb_load_text(None, t, len(t), 5, 10, 1, C.byref(r)) == _lib.PSG_ERR_ARG
    off = np.zeros(2, np.uint64)
    idx = np.zeros(1, np.uint64)
    y = np.zeros(1, np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # room for no entry: PSG_ERR_SIZE
    assert ok(t, len(t), 5, 10, 1, p(off), p(idx), None, p(y), 1, 0, C.byref(r)) == _lib.PSG_ERR_SIZE
    assert ok(t, len(t), 5, 10, 1, p(off), p(idx), None, p(y), 0, 1, C.byref(r)) == _lib.PSG_ERR_SIZE
    assert ok(t, len(t), 5, 10, 1, p(off), None, None, p(y), 1, 1, C.byref(r)) == _lib.PSG_ERR_ARG
    assert ok(t, len(t), 5, 10, 1, p(off), p(idx), None, p(y), 1, 1, C.byref(r)) == _lib.PSG_OK
    assert (int(off[1]), int(idx[0]), float(y[0])) == (1, 1, 1.0)
