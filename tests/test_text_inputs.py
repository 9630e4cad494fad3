"""CPU: the inputs of test_text_edges_gpu.py (text_inputs) have the structure
those tests rely on, recomputed here from the bytes alone, line by line and
token by token as text_ref cuts them; and the host parse
(psg_text_parse_host) equals the restatement on every one of them, so the
values the device is held to are what a correct implementation gives."""
import bisect
import itertools
import re

import numpy as np
import pytest

import text_inputs as I
import text_ref as T
from test_text import check

FORMATS = I.FORMATS
TOKEN = {T.LIBSVM: re.compile(rb"[^ \t\r\n]+"), T.ADFEA: re.compile(rb"[^ :]+")}


def structure(text, fmt, cross=True):
    """(line starts, newline places, token starts, slow token starts, lines):
    plain Python over the bytes.  Lines by fgets' rule with the text's end
    closing the last; a token is slow by psg.h's grammar (text_ref.fast_*)."""
    starts, nls, toks, slow = [], [], [], []
    at = 0
    lines = T.lines_of(text, True)
    for l in lines:
        starts.append(at)
        if l.endswith(b"\n"):
            nls.append(at + len(l) - 1)
        found = [(m.start(), m.group()) for m in TOKEN[fmt].finditer(l)]
        assert [t for _, t in found] == T.tokens_of(l, fmt)
        for i, (s, t) in enumerate(found):
            toks.append(at + s)
            if fmt == T.LIBSVM:
                if i == 0:
                    is_slow = not T.fast_float(t)
                else:
                    c = t[:T.MAX_FIELD + 1].find(b":")
                    is_slow = len(t) > T.MAX_FIELD if c < 0 else \
                        not (T.fast_key(t[:c]) and T.fast_float(t[c + 1:]))
            else:
                is_slow = (i == 2 and not T.fast_label(t)) or \
                    (i >= 3 and i % 2 == 1 and (len(t) > T.MAX_FIELD or not T.fast_key(t)))
            if is_slow:
                slow.append(at + s)
        at += len(l)
    assert not cross or len(slow) == T.slow_tokens(text, fmt)
    return starts, nls, toks, slow, lines


def per_lane(places):
    lane = I.geometry()[2]
    return max(np.bincount(np.array(places, np.int64) // lane)) if places else 0


def host(case):
    """psg_text_parse_host == text_ref.parse on the case, bit for bit."""
    return check(case.text, case.fmt, case.max_rows, case.final)


def test_skipped_pairs_and_geometry():
    assert I.SKIPPED == (("order_edges", T.ADFEA), ("two_bad/order", T.ADFEA),
                         ("lane_dense/newline_token", T.LIBSVM))
    assert I.order_edges(T.ADFEA) == []
    assert "order" not in I.mechanisms(T.ADFEA) and "order" in I.mechanisms(T.LIBSVM)
    assert not any("nl_token" in c.name for c in I.lane_dense(T.LIBSVM))
    c, w, lane = I.geometry()
    assert (c, c) == (4 * w, 256 * lane) and lane >= 16


@pytest.mark.parametrize("nc", I.MANY_CHUNKS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_many_chunks(fmt, nc):
    c = I.geometry()[0]
    plain, cut, bad = I.many_chunks(fmt, nc)
    text, k = plain.text, plain.claims
    assert (plain.name, cut.name, bad.name) == ("plain", "cut", "bad")
    assert -(-len(text) // c) == nc == k["nc"]
    assert k["per"] == -(-nc // 256) == {256: 1, 257: 2, 513: 3, 516: 3}[nc]
    starts, nls, toks, slow, lines = structure(text, fmt, cross=False)
    assert len(lines) == k["rows"] and text.endswith(b"\n")
    # the newline-free spans, from the newline places alone
    per, free, holding = k["per"], [], 0
    for t in range(256):
        b, e = min(t * per, nc), min(t * per + per, nc)
        holding += b < e
        if b < e and not any(p < e * c for p in nls[bisect.bisect_left(nls, b * c):][:1]):
            free.append(t)
    assert free == k["free"] and 256 - holding == k["empty"]
    assert holding == -(-nc // per) and (nc != 516 or (holding, k["empty"]) == (172, 84))
    run = max(len(list(g)) for _, g in itertools.groupby(enumerate(free), lambda p: p[1] - p[0]))
    assert run >= 3
    lo, hi = starts[k["long_row"]], starts[k["long_row"] + 1]
    assert 57 * 1024 < hi - lo < T.MAX_LINE - 1
    # every free span starts at a span boundary inside the long line
    assert all(lo < t * per * c and (t + 1) * per * c <= hi for t in free)
    # short fast lines otherwise; the slow ones in the last quarter
    assert max(len(l) for i, l in enumerate(lines) if i != k["long_row"]) < 600
    assert len(k["slow_rows"]) == 3 and min(slow) >= 3 * (len(text) // 4)
    assert {bisect.bisect_left(nls, s) for s in slow} == set(k["slow_rows"])
    r = host(plain)
    assert (r.rows, r.bad_line, r.consumed, r.slow_tokens) == (k["rows"], -1, len(text), len(slow))
    # the same text cut by max_rows inside the last quarter
    assert cut.text is text and cut.claims["consumed"] == starts[cut.max_rows]
    assert 3 * (len(text) // 4) < cut.claims["consumed"] < len(text)
    r = host(cut)
    assert (r.rows, r.bad_line, r.consumed) == (cut.max_rows, -1, cut.claims["consumed"])
    # ... and with one ':' of a line there made an 'x'
    diff = [i for i in range(len(text)) if text[i] != bad.text[i]] if text != bad.text else []
    assert len(bad.text) == len(text) and len(diff) == 1
    assert (text[diff[0]:diff[0] + 1], bad.text[diff[0]:diff[0] + 1]) == (b":", b"x")
    kb = bad.claims
    assert bisect.bisect_left(nls, diff[0]) == kb["bad"] and kb["consumed"] == starts[kb["bad"] + 1]
    assert 3 * (len(text) // 4) < starts[kb["bad"]] and kb["bad"] not in k["slow_rows"]
    r = host(bad)
    assert (r.rows, r.bad_line, r.consumed) == (kb["bad"], kb["bad"], kb["consumed"])
    rest = check(bad.text[r.consumed:], fmt)
    assert rest.bad_line == -1 and rest.rows == k["rows"] - kb["bad"] - 1


@pytest.mark.parametrize("fmt", FORMATS)
def test_wave_gaps(fmt):
    c, w, _ = I.geometry()
    (case,) = I.wave_gaps(fmt)
    text, k = case.text, case.claims
    _, nls, toks, _, lines = structure(text, fmt)
    assert 6 * c <= len(text) < 7 * c and len(lines) == k["rows"]
    kinds = {min(3, round(len(l) / (1.1 * w))) for l in lines}
    assert kinds == {0, 1, 2, 3}
    pairs, late = set(), False
    for ch in range(len(text) // c):
        wave_of = lambda p: (p - ch * c) // w
        nl = [[p for p in nls if ch * c <= p < (ch + 1) * c and wave_of(p) == i] for i in range(4)]
        tk = [[p for p in toks if ch * c <= p < (ch + 1) * c and wave_of(p) == i] for i in range(4)]
        for w0 in range(4):
            for w1 in range(w0 + 1, 4):
                if nl[w0] and not any(nl[w0 + 1:w1]) and tk[w1] and (not nl[w1] or tk[w1][0] < nl[w1][0]):
                    pairs.add((w0, w1))
        late |= bool(nl[3]) and not (nl[0] or nl[1] or nl[2])
    assert sorted(pairs) == k["pairs"] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert late and k["late"]
    r = host(case)
    assert (r.rows, r.bad_line) == (k["rows"], -1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_lane_dense(fmt):
    c, w, lane = I.geometry()
    cases = I.lane_dense(fmt)
    nl_places, ts_places, most_nl, most_ts, most_slow, nl_tokens = set(), set(), 0, 0, 0, []
    for case in cases:
        text, k = case.text, case.claims
        _, nls, toks, slow, lines = structure(text, fmt)
        assert sorted({p % lane for p in nls}) == k["nl_places"]
        assert sorted({p % lane for p in toks}) == k["ts_places"]
        assert (per_lane(nls), per_lane(toks)) == (k["nl_in_lane"], k["ts_in_lane"])
        nl_places |= set(k["nl_places"])
        ts_places |= set(k["ts_places"])
        most_nl, most_ts = max(most_nl, k["nl_in_lane"]), max(most_ts, k["ts_in_lane"])
        most_slow = max(most_slow, per_lane(slow))
        r = host(case)
        assert r.bad_line == k.get("bad", -1)
        if "slow_at" in k:
            assert k["slow_at"] in slow
        if "nl_token" in k:
            p = k["nl_token"]
            assert text[p - 1:p + 1] == b" \n" and p in toks and p in nls
            assert int(np.searchsorted(nls, p)) == k["bad"] and r.consumed == p + 1
            nl_tokens.append((p % lane, p % w, p % c))
            assert check(text[r.consumed:], fmt).bad_line == -1
    everywhere = set(range(lane))
    if fmt == T.LIBSVM:
        assert nl_places == everywhere and most_nl == 8 and most_slow >= 5
        assert len(cases) == lane
    else:
        assert ts_places == everywhere and most_ts == 8 and most_slow >= 5
        # first and last byte of a chunk, of a wave only, of a lane only
        assert nl_tokens == [(0, 0, 0), (lane - 1, w - 1, c - 1), (0, 0, w), (lane - 1, w - 1, 2 * w - 1),
                             (0, 5 * lane, w + 5 * lane), (lane - 1, 6 * lane - 1, w + 6 * lane - 1)]
        # without the rejected lines: 4 valid slow tokens in a lane
        assert max(per_lane(structure(x.text, fmt)[3]) for x in cases[:lane]) == 4


@pytest.mark.parametrize("fmt", FORMATS)
def test_text_ends(fmt):
    c, _, lane = I.geometry()
    cases = I.text_ends(fmt)
    seen = set()
    for case in cases:
        text, k = case.text, case.claims
        n = len(text)
        assert n == k["nbytes"] and text.endswith(b"\n") == k["ends_nl"]
        whole = text.count(b"\n")
        if not k["ends_nl"]:  # the middle of a number: its last two bytes are token bytes, the last a digit
            tail = T.lines_of(text, True)[-1]
            assert T.tokens_of(tail[-1:], fmt) and T.tokens_of(tail[-2:-1], fmt) and tail[-1:].isdigit()
        assert k["rows"] == whole + (1 if case.final and not k["ends_nl"] else 0)
        seen.add((n, k["ends_nl"], case.final))
        r = host(case)
        assert (r.rows, r.bad_line) == (k["rows"], -1)
        assert r.consumed == (n if case.final or k["ends_nl"] else text.rindex(b"\n") + 1)
    lengths = {q * lane + d for q in (5, 256 + 7) for d in (0, 1, lane - 1)} | \
              {q * c + d for q in (1, 2) for d in (-1, 0, 1)}
    assert seen == set(itertools.product(lengths, (True, False), (True, False)))
    assert {n % lane for n in lengths} >= {0, 1, lane - 1} and len(lengths) == 12


def rejected_by(l, fmt):
    """The mechanisms that reject line l, each judged on its own."""
    how = set()
    if len(l) >= T.MAX_LINE - 1:
        how.add("long")
    if b"\0" in l:
        how.add("nul")
    tok = T.tokens_of(l.replace(b"\0", b""), fmt)
    if fmt == T.LIBSVM:
        if not tok or any(b":" not in t for t in tok[1:]):
            how.add("sight")
        pairs = [t.split(b":", 1) for t in tok[1:] if b":" in t]
        if not T.strtofloat(tok[0])[1] or any(not T.strtou64(a)[1] or not T.strtofloat(b)[1]
                                              for a, b in pairs):
            how.add("libc")
        keys = [T.strtou64(a)[0] for a, _ in pairs]
        if any(x > y for x, y in zip(keys, keys[1:])):
            how.add("order")
    else:
        if len(tok) < 3:
            how.add("sight")
        elif not T.strtoi32(tok[2])[1] or any(not T.strtou64(t)[1] for t in tok[3::2]):
            how.add("libc")
    return how


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_bad(fmt):
    c = I.geometry()[0]
    cases = I.two_bad(fmt)
    mech = ("sight", "libc", "order", "long", "nul") if fmt == T.LIBSVM else ("sight", "libc", "long", "nul")
    assert [x.name for x in cases] == [a + "," + b for a in mech for b in mech]
    for case in cases:
        text, k = case.text, case.claims
        starts, _, _, _, lines = structure(text, fmt)
        assert len(text) >= 4 * c and len(lines) == k["rows"]
        bad = [i for i, l in enumerate(lines) if T.parse_line(l, fmt) is None]
        assert bad == [k["bad"], k["bad2"]]
        first, second = case.name.split(",")
        assert rejected_by(lines[bad[0]], fmt) == {first}
        assert rejected_by(lines[bad[1]], fmt) == {second}
        # in different chunks: the first ends before the chunk the second starts in
        assert (starts[bad[0]] + len(lines[bad[0]]) - 1) // c < starts[bad[1]] // c
        assert k["consumed"] == starts[bad[0] + 1] and k["consumed2"] == starts[bad[1] + 1]
        r = host(case)
        assert (r.rows, r.bad_line, r.consumed) == (k["bad"], k["bad"], k["consumed"])
        r2 = check(text[k["consumed"]:], fmt)
        assert (r2.bad_line, r2.consumed) == (k["bad2"] - k["bad"] - 1, k["consumed2"] - k["consumed"])
        r3 = check(text[k["consumed2"]:], fmt)
        assert r3.bad_line == -1 and r3.rows == k["rows"] - k["bad2"] - 1 > 0


def test_order_edges():
    cases = I.order_edges()
    assert [x.name for x in cases] == [
        "descending_after_0", "boundary_over_0", "descending_after_1", "boundary_over_1",
        "descending_after_300", "boundary_over_300", "descending_last", "equal"]
    for case in cases:
        text, k = case.text, case.claims
        lines = T.lines_of(text, True)
        keys = [[T.strtou64(t.split(b":")[0])[0] for t in T.tokens_of(l, T.LIBSVM)[1:]] for l in lines]
        down = [i for i, ks in enumerate(keys) if any(a > b for a, b in zip(ks, ks[1:]))]
        assert down == ([k["bad"]] if k["bad"] >= 0 else [])
        assert sum(map(len, keys)) > 256  # more than one workgroup of order_kernel
        full = [i for i, ks in enumerate(keys) if ks]
        if case.name.startswith("descending_after"):
            i = k["bad"]
            assert keys[i][-2] > keys[i][-1] and all(not keys[j] for j in range(i - k["empty"], i))
            assert keys[i - k["empty"] - 1]  # ... and entries before them: the offsets repeat
        if case.name.startswith("boundary_over"):
            i = next(i for i, ks in enumerate(keys) if ks and ks[-1] == I.K64)
            j = i + k["empty"] + 1
            assert all(not keys[x] for x in range(i + 1, j)) and keys[i][-1] > keys[j][0]
        if case.name == "descending_last":
            assert k["bad"] == len(lines) - 1 and keys[-1][-2] > keys[-1][-1]
        if case.name == "equal":
            assert any(a == b for ks in keys for a, b in zip(ks, ks[1:]))
        # by chance too: some good row ends above the next one's first index
        assert any(keys[a][-1] > keys[b][0] for a, b in zip(full, full[1:]))
        r = host(case)
        assert r.bad_line == k["bad"] and (k["bad"] >= 0 or r.rows == len(lines))


@pytest.mark.parametrize("fmt", FORMATS)
def test_row_cuts(fmt):
    c, w, lane = I.geometry()
    cases = I.row_cuts(fmt)
    assert [x.name for x in cases] == ["lane", "wave", "chunk", "lines-1", "lines", "lines+1"]
    text = cases[0].text
    starts, nls, _, _, lines = structure(text, fmt)
    starts.append(len(text))
    n = len(lines)
    for case in cases:
        k = case.claims
        assert case.text is text and k["lines"] == n and k["rows"] == min(case.max_rows, n)
        cut = k["cut"]
        assert cut == starts[k["rows"]]
        if case.name == "lane":  # the line before ends in this lane, the line cut off too
            assert cut % lane and (cut - 1) // lane == cut // lane == (starts[k["rows"] + 1] - 1) // lane
        if case.name == "wave":
            assert cut % w == 0 and cut % c
        if case.name == "chunk":
            assert cut % c == 0 and cut > 0
        r = host(case)
        assert (r.rows, r.consumed, r.bad_line) == (k["rows"], cut, -1)
    assert [x.max_rows for x in cases[3:]] == [n - 1, n, n + 1]


@pytest.mark.parametrize("fmt", FORMATS)
def test_converter_sweep(fmt):
    cases = I.converter_sweep(fmt)
    tokens, fields = 0, set()
    for case in cases:
        text, k = case.text, case.claims
        _, _, toks, slow, lines = structure(text, fmt)
        parsed = 0
        for l in lines:
            assert len(l) < T.MAX_LINE - 1
            tok = T.tokens_of(l, fmt)
            if fmt == T.LIBSVM:
                parsed += len(tok)
                keys = [T.strtou64(t.split(b":")[0])[0] for t in tok[1:]]
                fields |= {tok[0]} | {t.split(b":")[1] for t in tok[1:]}
            else:
                parsed += 1 + len(tok[3::2])
                keys = [T.strtou64(t)[0] for t in tok[3::2]]
                fields.add(tok[2])
            fields |= {b"k%d" % len(t.split(b":")[0]) for t in (tok[1:] if fmt == T.LIBSVM else tok[3::2])}
            assert keys == sorted(keys)
        assert (parsed - len(slow), len(slow)) == (k["fast"], k["slow"]) and k["fast"] and k["slow"]
        assert 1000 <= parsed <= 6000
        tokens += parsed
        r = host(case)
        assert (r.rows, r.bad_line, r.slow_tokens) == (k["rows"], -1, k["slow"])
    assert tokens <= 30000
    assert {b"k%d" % d for d in range(1, 21)} <= fields
    text = b"".join(x.text for x in cases)
    for key in (I.K64, I.K64 + 1, 10 ** 19, 10 ** 20 - 1):
        assert b" %d:" % key in text
    if fmt == T.ADFEA:
        assert {b"0", b"-0", b"1", b"-1", b"999999999", b"-999999999", b"1000000000",
                b"-1000000000"} <= fields
        return
    for w in (0, 1, 9, 10, (1 << 24) - 1, 1 << 24, (1 << 24) + 1):
        for frac in range(12):
            for neg in (False, True):
                assert I.decimal(w, frac, neg).encode() in fields
    sizes = {len(f) for f in fields if f.startswith((b"0000", b"-0000")) or f.endswith(b"0000")}
    assert {T.MAX_FIELD - 1, T.MAX_FIELD, T.MAX_FIELD + 1} <= sizes
