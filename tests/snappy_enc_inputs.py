"""TEST INFRASTRUCTURE: inputs of the snappy encoder's tests (the host twin
in tests/test_snappy_compress.py, the device encoder in
tests/test_snappy_compress_gpu.py), every one from splitmix64 as pin_cases
builds its own, and the walk that checks what a stream is made of.

STEP, FRAGMENT and MAX_COPY mirror psg_snappy_enc.h (kStep, kFragment,
kMaxCopy): the encoder walks a 64 KB fragment in steps of 256 positions and a
position finds its match among the positions of earlier steps only.
"""
import numpy as np

import pin_cases as P

STEP, FRAGMENT, MAX_COPY = 256, 65536, 64
EDGE_LENGTHS = (0, 1, 3, 4, 15, 16, 17, 60, 61)
MATCH_LENGTHS = (3, 4, 11, 12, 64, 65)
_cache = {}


def periodic(n, period=7):
    return (bytes(range(65, 65 + period)) * (n // period + 1))[:n]


def repeat_at(distance, seed):
    """`distance` random bytes, their first 8 again, then 8 that break the
    match: one 8-byte match at exactly that distance."""
    base = P.random_bytes(seed, distance)
    return base + base[:8] + bytes([base[8] ^ 0xFF]) + P.random_bytes(seed + 1, 7)


def match_of(m, seed):
    """600 random bytes, then bytes [100, 100 + m) of them again at position
    600 (step 2; the source lies in step 0), cut off on both sides by a byte
    that differs: one match of exactly m bytes."""
    r = bytearray(P.random_bytes(seed, 600))
    r[599] = r[99] ^ 0xFF
    return bytes(r) + bytes(r[100:100 + m]) + bytes([r[100 + m] ^ 0xFF]) + P.random_bytes(seed + 1, 20)


def source_at_step_start(inclusive, seed):
    """A 16-byte match at position 300 whose source ends right before
    position 256, step 1's first (inclusive: whose last byte is position
    256)."""
    r = bytearray(P.random_bytes(seed, 300))
    s = 256 - 16 + (1 if inclusive else 0)
    r[299] = r[s - 1] ^ 0xFF
    return bytes(r) + bytes(r[s:s + 16]) + bytes([r[s + 16] ^ 0xFF]) + P.random_bytes(seed + 1, 20)


def edge_inputs():
    """[(name, bytes)]: the smallest inputs that hit each seam of the format
    and of the rule; built once, read only."""
    if "edge" not in _cache:
        out = [("len%d" % n, P.random_bytes(40060 + n, n)) for n in EDGE_LENGTHS]
        # the literal tag's 1-, 2- and 3-byte length forms
        out += [("rand%d" % n, P.random_bytes(43000 + n, n)) for n in (256, 257, FRAGMENT)]
        # fragment seams: a match that would run across one is cut there
        out += [("periodic%d" % n, periodic(n)) for n in (FRAGMENT - 1, FRAGMENT, FRAGMENT + 1,
                                                          2 * FRAGMENT + 1)]
        # the copy-1 / copy-2 seam of the offset
        out += [("at%d" % d, repeat_at(d, 43100 + d)) for d in (2047, 2048)]
        # no match, the minimum match, copy-1's length limit, one and two copies
        out += [("match%d" % m, match_of(m, 43200 + 2 * m)) for m in MATCH_LENGTHS]
        # the step's own seams
        out += [("step%d" % n, periodic(n, 5)) for n in (STEP - 1, STEP, STEP + 1, 2 * STEP - 1,
                                                        2 * STEP, 2 * STEP + 1)]
        out += [("src_before_step", source_at_step_start(False, 43400)),
                ("src_into_step", source_at_step_start(True, 43410))]
        _cache["edge"] = out
    return _cache["edge"]


def all_inputs():
    """The pinned cases and the edge inputs, [(name, bytes)]; names unique."""
    if "all" not in _cache:
        pinned = [("pin_" + c.name, c.data) for c in P.snappy_cases()]
        _cache["all"] = pinned + edge_inputs()
        assert len({n for n, _ in _cache["all"]}) == len(_cache["all"])
    return _cache["all"]


def fuzz_input(seed):
    """Input `seed` of the fuzz: 0 .. 200,000 bytes over an alphabet of 1, 2,
    4 or 256 symbols, or 8-byte records drawn from a pool of 50."""
    d = P.splitmix64(44000 + seed, 3)
    n = int(d[0] % np.uint64(200001))
    kind = seed % 5
    if kind == 4:
        pool = P.splitmix64(45000 + seed, 50)
        pick = (P.splitmix64(46000 + seed, n // 8 + 1) % np.uint64(50)).astype(np.int64)
        return P.le_bytes(pool[pick])[:n]
    raw = np.frombuffer(P.random_bytes(45000 + seed, n), np.uint8)
    bits = (0, 1, 2, 8)[kind]
    return (raw >> np.uint8(8 - bits)).astype(np.uint8).tobytes() if bits else bytes(n)


def elements(stream):
    """pin_cases.snappy_elements, with the walk required to end at the
    stream's end: (declared length, [(kind, length, offset, output position)])."""
    ulen, el = P.snappy_elements(stream)
    assert ulen is not None, "bad preamble"
    out, x, stop = [], 0, max(1, (ulen.bit_length() + 6) // 7)
    for pos, kind, ln, field in el:
        out.append((kind, ln, field if kind else 0, x))
        x += ln
        stop = pos + (field + ln if kind == 0 else 1 + kind)
    assert stop == len(stream), "the element walk stops at %d of %d" % (stop, len(stream))
    return ulen, out


def check_structure(stream, n):
    """What every stream of the encoder holds to: the declared length, only
    literal / copy-1 / copy-2 elements, offsets below 65536, no element across
    a fragment seam and no copy from before its fragment's start."""
    ulen, el = elements(stream)
    assert ulen == n
    assert sum(e[1] for e in el) == n
    for kind, ln, off, x in el:
        assert kind in (0, 1, 2), "copy-4"
        assert x // FRAGMENT == (x + ln - 1) // FRAGMENT, "an element crosses a fragment seam"
        if kind:
            assert 1 <= off < 65536 and 4 <= ln <= MAX_COPY
            assert x - off >= x // FRAGMENT * FRAGMENT, "a copy reaches before its fragment"
    return el
