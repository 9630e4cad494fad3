"""Inputs of the text ingest's edge tests (test_text_inputs.py on the CPU,
test_text_edges_gpu.py on the device): texts that drive the parts of
psg_text.hip no earlier test reaches, one builder per part.  A builder returns
Cases: the text, the call's arguments and the *claims*, the structural facts
the case exists for, which test_text_inputs.py recomputes from the bytes.

All places are in units of the kernels' geometry: a workgroup takes a chunk
(psg_text_chunk()), a wave a quarter of it, a lane 1/256 of it."""
import functools
import itertools
import random
from collections import namedtuple

import numpy as np

import text_ref as T
from test_text_gpu import line, placed
from parameter_server_amd.worker import text_chunk

Case = namedtuple("Case", "name text fmt max_rows final claims")
FORMATS = (T.LIBSVM, T.ADFEA)
K64 = (1 << 64) - 1

# What a format cannot express, as (builder, format): the builder returns no
# case for it, and test_text_inputs.py holds this list exactly.
SKIPPED = (
    ("order_edges", T.ADFEA),            # parseAdfea has no order rule: no key is compared
    ("two_bad/order", T.ADFEA),          # ... so no line is rejected by descending keys
    ("lane_dense/newline_token", T.LIBSVM),  # '\n' is a LIBSVM delimiter, never a token
)


def geometry():
    """(chunk, wave, lane) in bytes."""
    c = text_chunk()
    return c, c // 4, c // 256


def case(name, text, fmt, max_rows=None, final=True, **claims):
    return Case(name, text, fmt, max_rows, final, claims)


# ---- the bytes' structure, vectorised (the CPU test recomputes it per line) ----
def _bytes(text):
    return np.frombuffer(text, np.uint8)


def newline_places(text):
    return np.flatnonzero(_bytes(text) == 10)


def token_starts(text, fmt):
    """A token byte after a delimiter, a '\\n' or the start of the text."""
    a = _bytes(text)
    delims = np.frombuffer(b" \t\r\n" if fmt == T.LIBSVM else b" :", np.uint8)
    d = np.isin(a, delims)
    prev = np.concatenate((np.array([10], np.uint8), a[:-1]))
    return np.flatnonzero(~d & ((prev == 10) | np.isin(prev, delims)))


def join_to(lines, total):
    """The lines as one text of `total` bytes: blanks lead line 0."""
    size = sum(map(len, lines))
    assert size <= total
    return b" " * (total - size) + b"".join(lines)


def wide_line(fmt, i, nf):
    """A fast-grammar line of nf entries whose fields are long (trailing
    fraction zeros, long slot ids), so a megabyte holds few tokens."""
    keys = sorted((i * 1000003 + j + 1) * 1844674407370955 % (1 << 64) for j in range(nf))
    if fmt == T.LIBSVM:
        return ("%d " % (i % 3 - 1) + " ".join("%d:%d.%06d%s" % (k, j % 7, (k >> 7) % 1000000, "0" * 50)
                                               for j, k in enumerate(keys)) + "\n").encode()
    return ("%d 1 %d " % (i, i % 2) + " ".join("%d:%058d" % (k, j) for j, k in enumerate(keys))
            + "\n").encode()


def sized_line(fmt, i, nbytes, make=line):
    """make(fmt, i, nf) with nf chosen for about nbytes."""
    nf = 64
    for _ in range(3):  # the bytes per entry grow a little with nf
        nf = max(1, int(nf * nbytes / len(make(fmt, i, nf))))
    return make(fmt, i, nf)


SLOW_LINE = {T.LIBSVM: b"1e0 3:1e-3 7:+1 9:0x1p-2\n", T.ADFEA: b"a b +1 +7:1 +9:2\n"}


# ---- 1. chunk_scan_kernel with more than one chunk per lane ---------------------
MANY_CHUNKS = (256, 257, 513, 516)


def free_spans(text, nc):
    """The spans [t * per, (t + 1) * per) of chunk_scan_kernel's lanes that
    hold chunks but no newline, and how many lanes hold no chunk."""
    c = geometry()[0]
    per = -(-nc // 256)
    nl = newline_places(text)
    free, empty = [], 0
    for t in range(256):
        b = min(t * per, nc)
        e = min(b + per, nc)
        if b == e:
            empty += 1
        elif np.searchsorted(nl, b * c) == np.searchsorted(nl, min(e * c, len(text))):
            free.append(t)
    return per, free, empty


@functools.lru_cache(maxsize=2)
def _many_chunks_text(fmt, nc):
    c = geometry()[0]
    total = nc * c - c // 2 + 5
    long_line = sized_line(fmt, 5, 59 * 1024)
    assert 57 * 1024 < len(long_line) < T.MAX_LINE - 1
    lines, size, i, slow_rows, long_row = [], 0, 0, [], None
    while size < total - 400:
        if long_row is None and size >= 2 * total // 5:
            long_row, l = len(lines), long_line
        elif len(slow_rows) < 3 and size >= (13 + len(slow_rows)) * (total // 16):
            slow_rows.append(len(lines))
            l = SLOW_LINE[fmt]
        else:
            l = wide_line(fmt, i, 1 + i % 2)
        lines.append(l)
        size += len(l)
        i += 1
    text = join_to(lines, total)
    assert (len(text) + c - 1) // c == nc
    return text, len(lines), long_row, tuple(slow_rows)


def many_chunks(fmt, nc):
    """plain / cut (max_rows inside the last quarter) / bad (one byte changed
    there: a LIBSVM pair loses its ':', an ADFEA key takes its slot in)."""
    text, rows, long_row, slow_rows = _many_chunks_text(fmt, nc)
    per, free, empty = free_spans(text, nc)
    nl = newline_places(text)
    facts = dict(nc=nc, per=per, free=free, empty=empty, rows=rows, long_row=long_row,
                 slow_rows=list(slow_rows))
    cut = int(np.searchsorted(nl, 15 * (len(text) // 16)))  # the lines that end before that place
    colon = text.index(b":", 29 * (len(text) // 32))
    bad = int(np.searchsorted(nl, colon))
    assert bad not in slow_rows and bad < cut
    mutated = text[:colon] + b"x" + text[colon + 1:]
    return [case("plain", text, fmt, **facts),
            case("cut", text, fmt, max_rows=cut, consumed=int(nl[cut - 1]) + 1, **facts),
            case("bad", mutated, fmt, bad=bad, consumed=int(nl[bad]) + 1, **facts)]


# ---- 2. the carry between the waves of one chunk --------------------------------
def wave_facts(text, fmt):
    """(pairs, late): the (w0, w1) for which some whole chunk has a newline in
    wave w0, none in the waves between, and in wave w1 a token start before any
    newline of w1; whether some chunk's first newline lies in its last wave."""
    c, w, _ = geometry()
    nl, ts = newline_places(text), token_starts(text, fmt)
    pairs, late = set(), False
    for k in range(len(text) // c):
        nls = [nl[(nl >= k * c + i * w) & (nl < k * c + (i + 1) * w)] for i in range(4)]
        tss = [ts[(ts >= k * c + i * w) & (ts < k * c + (i + 1) * w)] for i in range(4)]
        for w0, w1 in itertools.combinations(range(4), 2):
            if nls[w0].size and not any(nls[i].size for i in range(w0 + 1, w1)) and tss[w1].size \
                    and (not nls[w1].size or tss[w1][0] < nls[w1][0]):
                pairs.add((w0, w1))
        late |= bool(nls[3].size) and not any(nls[i].size for i in range(3))
    return sorted(pairs), late


def wave_gaps(fmt):
    """About 6 chunks of lines of a short length or of about 1.1, 2.2 and 3.3
    waves, from the first seed whose text has every wave pair."""
    c, w, _ = geometry()
    want = sorted(itertools.combinations(range(4), 2))
    for seed in range(256):
        rng = np.random.default_rng(seed)
        lines, size = [], 0
        while size < 6 * c:
            kind = int(rng.integers(0, 8))
            i = len(lines)
            l = line(fmt, i, 1 + i % 3) if kind < 5 else sized_line(fmt, i, (kind - 4) * 1.1 * w)
            lines.append(l)
            size += len(l)
        text = b"".join(lines)
        pairs, late = wave_facts(text, fmt)
        if pairs == want and late:
            return [case("seed%d" % seed, text, fmt, pairs=pairs, late=late, rows=len(lines))]
    raise AssertionError("no seed gives every wave pair")


# ---- 3. the lane's bit masks ----------------------------------------------------
def lane_facts(text, fmt):
    """Per lane: the places (byte mod lane) of newlines and of token starts,
    and the most of each that one lane holds."""
    lane = geometry()[2]
    nl, ts = newline_places(text), token_starts(text, fmt)
    most = lambda a: int(np.bincount(a // lane).max()) if a.size else 0
    return dict(nl_places=sorted(set((nl % lane).tolist())), ts_places=sorted(set((ts % lane).tolist())),
                nl_in_lane=most(nl), ts_in_lane=most(ts))


def lane_dense(fmt):
    """The shortest legal material behind 0 .. lane - 1 leading blanks, a run
    of valid slow tokens at a lane's first byte, and the ADFEA lines that end
    " \\n" (the '\\n' is a key token: rejected) with that '\\n' at the first and
    the last byte of a lane, a wave and a chunk."""
    c, w, lane = geometry()
    rng = np.random.default_rng(21)
    out = []
    if fmt == T.LIBSVM:
        body = [b"1\n" * 24]
        while sum(map(len, body)) < c + c // 3 or sum(map(len, body)) % lane:
            body.append(b"1\n" if rng.integers(0, 10) < 7 else b"0.5\n")
        slow = b"+1\n" * 5 + b"1\n" * 8  # 5 slow labels in lane - 1 bytes
        tail = [b"1\n" if rng.integers(0, 10) < 7 else b"0.5\n" for _ in range(c // 3)]
    else:
        body = []
        while sum(map(len, body)) < c + c // 3 or sum(map(len, body)) % lane:
            k = int(rng.integers(1, 13))
            body.append(b"a b 1" + b" 1:1" * k + b"\n")
        slow = b"a b +1 +1 1 +1 1 +1 1 +1 1\n"  # valid: 4 slow tokens in a lane at the most
        tail = [b"a b 1" + b" 1:1" * int(rng.integers(1, 13)) + b"\n" for _ in range(c // 12)]
    at = sum(map(len, body))
    for shift in range(lane):
        text = b" " * shift + b"".join(body) + slow + b"".join(tail)
        assert len(text) > 2 * c
        first_slow = shift + at + (0 if fmt == T.LIBSVM else 4)  # ADFEA: behind "a b "
        out.append(case("shift%d" % shift, text, fmt, slow_at=first_slow, **lane_facts(text, fmt)))
    if fmt == T.LIBSVM:
        return out  # SKIPPED: no LIBSVM '\n' is a token
    # one-byte tokens libc rejects: label, key, slot, key, ... 5 slow tokens in
    # one lane; the line is rejected, so it is the load's last
    head = b"".join(body)
    five = b"a b x y 1 z 1 w 1 v 1\n"
    text = head + b" " * (lane - 4) + five
    assert (len(text) - len(five) + 4) % lane == 0
    out.append(case("slow5", text, fmt, slow_at=len(text) - len(five) + 4, bad=len(body),
                    **lane_facts(text, fmt)))
    lines = [line(fmt, i, 2) for i in range(3 * c // 40)]
    t = len(lines) // 6
    lines[t] = b"a b 1 1:1 \n"
    assert sum(map(len, lines[:t])) < c and sum(map(len, lines)) > 2 * c + c // 4
    for name, at in (("chunk_first", 2 * c), ("chunk_last", 2 * c - 1), ("wave_first", c + w),
                     ("wave_last", c + 2 * w - 1), ("lane_first", c + w + 5 * lane),
                     ("lane_last", c + w + 6 * lane - 1)):
        text = placed(fmt, lines, t, len(lines[t]) - 1, at)
        out.append(case("nl_token_" + name, text, fmt, nl_token=at, bad=t, **lane_facts(text, fmt)))
    return out


# ---- 4. where the text ends -----------------------------------------------------
def text_ends(fmt):
    """Lengths around a lane's and a chunk's multiples, ending in '\\n' or in
    the middle of a token (a LIBSVM value's fraction, an ADFEA key), each with
    `final` on and off."""
    c, _, lane = geometry()
    lines = [line(fmt, i, 1 + i % 3) for i in range(2 * c // 30 + 8)]
    last = line(fmt, 7, 1)
    mid = last[:last.index(b":") + 4] if fmt == T.LIBSVM else last[:last.index(b":") - 3]
    lengths = [k * lane + d for k in (5, 256 + 7) for d in (0, 1, lane - 1)] + \
              [k * c + d for k in (1, 2) for d in (-1, 0, 1)]
    out = []
    for n in lengths:
        for tail in (b"", mid):
            take, size = [], len(tail)
            for l in lines:
                if size + len(l) > n:
                    break
                take.append(l)
                size += len(l)
            assert n - size < 120
            text = join_to(take + [tail], n)
            for final in (True, False):
                out.append(case("%d%s%s" % (n, "+mid" if tail else "", "" if final else "-open"),
                                text, fmt, final=final, nbytes=n, ends_nl=not tail,
                                rows=len(take) + (1 if tail and final else 0)))
    return out


# ---- 5. the minimum over rejected lines -----------------------------------------
def bad_line(fmt, how, i):
    """A line that mechanism `how` alone rejects."""
    if how == "long":
        l = sized_line(fmt, i, T.MAX_LINE + 300)
        assert T.MAX_LINE - 1 <= len(l) < T.MAX_LINE + 1024
        return l
    return {T.LIBSVM: {"sight": b"1 5:1 4\n",        # a pair without ':'
                       "libc": b"1 5:1e 6:1\n",      # strtof stops at 'e'
                       "order": b"1 5:1 4:1\n",
                       "nul": b"1 5:1 6:1\0\n"},     # libc takes "1"; only the NUL rejects
            T.ADFEA: {"sight": b"a b\n",             # fewer than three tokens
                      "libc": b"a b 1 5:1 4\n",      # the key "4\n"
                      "nul": b"a b 1 5:1\0\n"}}[fmt][how]   # the slot id is not parsed


def mechanisms(fmt):
    return ("sight", "libc", "order", "long", "nul") if fmt == T.LIBSVM \
        else ("sight", "libc", "long", "nul")  # SKIPPED: two_bad/order


def two_bad(fmt):
    """Every ordered pair of mechanisms: the earlier line rejected by the
    first, the later, in another chunk, by the second; good lines around."""
    c = geometry()[0]
    out = []
    for first, second in itertools.product(mechanisms(fmt), repeat=2):
        good = (line(fmt, i, 2) for i in itertools.count())
        lines, size, bad = [], 0, []
        for how, gap in ((first, c + c // 2), (second, c + c // 3), (None, c + c // 4)):
            goal = size + gap
            while size < goal:
                lines.append(next(good))
                size += len(lines[-1])
            if how:
                bad.append((len(lines), size // c))
                lines.append(bad_line(fmt, how, 7))
                size += len(lines[-1])
        text = b"".join(lines)
        ends = np.cumsum([len(l) for l in lines])
        assert len(text) >= 4 * c and (ends[bad[0][0]] - 1) // c < bad[1][1]
        out.append(case(first + "," + second, text, fmt, bad=bad[0][0], bad2=bad[1][0],
                        consumed=int(ends[bad[0][0]]), consumed2=int(ends[bad[1][0]]),
                        rows=len(lines)))
    return out


# ---- 6. order_kernel's search over equal offsets ---------------------------------
def order_edges(fmt=T.LIBSVM):
    if fmt != T.LIBSVM:
        return []  # SKIPPED: order_edges
    good = [line(fmt, i, 8) for i in range(40)]  # 320 entries: more than one block of order_kernel
    out = []
    for empty in (0, 1, 300):
        lines = good[:30] + [b"1\n"] * empty + [b"1 5:1 4:1\n"] + good[30:]
        out.append(case("descending_after_%d" % empty, b"".join(lines), fmt, bad=30 + empty,
                        empty=empty))
        # the last index of a row above the first of the next: no order across rows
        lines = good[:30] + [b"1 7:1 %d:2\n" % K64] + [b"-1\n"] * empty + [b"1 3:1 4:1\n"] + good[30:]
        out.append(case("boundary_over_%d" % empty, b"".join(lines), fmt, bad=-1, empty=empty))
    out.append(case("descending_last", b"".join(good + [b"1 3:1 5:1 4:1\n"]), fmt, bad=40, empty=0))
    out.append(case("equal", b"".join(good[:20] + [b"1 5:1 5:2 6:3 6:4\n"] + good[20:]), fmt, bad=-1,
                    empty=0))
    return out


# ---- 7. max_rows cuts --------------------------------------------------------------
def starts_of(lines):
    return np.concatenate(([0], np.cumsum([len(l) for l in lines])))


def lead_to(lines, at):
    """Blanks lead the line before the last one that starts at or before
    `at`, so that this one starts at `at`; its number."""
    s = starts_of(lines)
    r = int(np.searchsorted(s, at, side="right")) - 1
    lines[r - 1] = b" " * int(at - s[r]) + lines[r - 1]
    return r


def row_cuts(fmt):
    """One text; max_rows so that the first byte not consumed lies between two
    lines of one lane, at a wave's and at a chunk's first byte, and at lines
    - 1, lines, lines + 1."""
    c, w, lane = geometry()
    short = [b"1\n", b"0.5\n"] * 40 if fmt == T.LIBSVM else [b"a b 1 1:1\n"] * 40
    lines = short + [line(fmt, i, 1 + i % 3) for i in range(3 * c // 50)]
    r_wave = lead_to(lines, c + w)
    r_chunk = lead_to(lines, 2 * c)
    starts = starts_of(lines)
    assert r_wave < r_chunk and starts[r_wave] == c + w and starts[r_chunk] == 2 * c
    # a line of the short run that ends in the lane it starts in, not at the lane's first byte
    r_lane = next(r for r in range(1, len(short))
                  if starts[r] % lane and starts[r] // lane == (starts[r + 1] - 1) // lane)
    text, n = b"".join(lines), len(lines)
    return [case(name, text, fmt, max_rows=r, cut=int(starts[min(r, n)]), rows=min(r, n), lines=n)
            for name, r in (("lane", r_lane), ("wave", r_wave), ("chunk", r_chunk),
                            ("lines-1", n - 1), ("lines", n), ("lines+1", n + 1))]


# ---- 8. the fast converters as the device compiles them --------------------------
def decimal(w, k, neg=False, lead=0, trail=0):
    """w / 10^k in the fast grammar's form, with `lead` zeros before it and
    `trail` more fraction zeros (a '.' is added for them where k == 0)."""
    d = "%0*d" % (k + 1, w)
    s = "0" * lead + (d[:-k] + "." + d[-k:] if k else d)
    if trail:
        s += ("" if k else ".") + "0" * trail
    return ("-" if neg else "") + s


def decimal_is_fast(s):
    """psg.h's rule, by arithmetic on the digits."""
    body = s.lstrip("-")
    whole, _, frac = body.partition(".")
    frac = frac.rstrip("0")
    return len(s) <= T.MAX_FIELD and int(whole + frac) <= 1 << 24 and len(frac) <= 10


def sweep_decimals(seed):
    rng = np.random.default_rng(seed)
    edge = [0, 1, 9, 10, (1 << 24) - 1, 1 << 24, (1 << 24) + 1]
    ws = edge + [int(x) for x in rng.integers(0, (1 << 24) + 1, 290)]
    out = [decimal(w, k, neg) for w in ws for k in range(12) for neg in (False, True)]
    for w, k, neg, size in itertools.product(edge, (0, 1, 10), (False, True),
                                             (T.MAX_FIELD - 1, T.MAX_FIELD, T.MAX_FIELD + 1)):
        plain = decimal(w, k, neg)
        out.append(decimal(w, k, neg, lead=size - len(plain)))
        out.append(decimal(w, k, neg, trail=size - len(plain) - (0 if k else 1)))
        assert len(out[-1]) == len(out[-2]) == size
    return out


def sweep_keys(seed):
    rng = random.Random(seed)
    keys = [0, K64 - 1, K64, K64 + 1, 10 ** 19, 10 ** 20 - 1, 18446744073709551609,
            18446744073709551620, 10 ** 20, int("9" * 25)]  # the last two: 21, 25 digits (slow)
    for d in range(1, 21):
        keys += [10 ** (d - 1), 10 ** d - 1] + [rng.randrange(10 ** (d - 1), 10 ** d) for _ in range(6)]
    return [str(k) for k in keys] + ["00000000000000000123", "000000000000000000123"]


def converter_sweep(fmt):
    """Texts of two entries a line, keys ascending as strtoull reads them."""
    keys = sweep_keys(31)
    value = lambda s: min(int(s), K64)
    out = []
    if fmt == T.LIBSVM:
        dec = sweep_decimals(32)
        lines, fast, slow = [], 0, 0
        for i, lab in enumerate(dec):
            k = sorted((keys[(2 * i) % len(keys)], keys[(2 * i + 7) % len(keys)]), key=value)
            v = (dec[(i * 7 + 3) % len(dec)], dec[(i * 11 + 5) % len(dec)])
            ok = [decimal_is_fast(lab)] + [len(k[j]) <= 20 and decimal_is_fast(v[j]) for j in (0, 1)]
            fast += sum(ok)
            slow += 3 - sum(ok)
            lines.append("%s %s:%s %s:%s\n" % (lab, k[0], v[0], k[1], v[1]))
            if len(lines) == 1500 or i + 1 == len(dec):
                out.append(case("part%d" % len(out), "".join(lines).encode(), fmt, fast=fast,
                                slow=slow, rows=len(lines)))
                lines, fast, slow = [], 0, 0
        return out
    rng = np.random.default_rng(33)
    labels = ["0", "-0", "1", "-1", "999999999", "-999999999", "1000000000", "-1000000000",
              "+1", "2147483647", "-2147483648", "000000001", "0000000001"]
    labels += ["%s%d" % ("-" if rng.integers(0, 2) else "", rng.integers(0, 10 ** int(rng.integers(1, 10))))
               for _ in range(200)]
    lines, fast, slow = [], 0, 0
    for i in range(3000):
        lab = labels[i % len(labels)]
        k = sorted((keys[(2 * i) % len(keys)], keys[(2 * i + 7) % len(keys)]), key=value)
        ok = [len(lab.lstrip("-")) <= 9 and not lab.startswith("+")] + [len(x) <= 20 for x in k]
        fast += sum(ok)
        slow += 3 - sum(ok)
        lines.append("%d 1 %s %s:%d %s:%d\n" % (i, lab, k[0], i % 10, k[1], i % 7))
        if len(lines) == 1500:
            out.append(case("part%d" % len(out), "".join(lines).encode(), fmt, fast=fast, slow=slow,
                            rows=len(lines)))
            lines, fast, slow = [], 0, 0
    return out
