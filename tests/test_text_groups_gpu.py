"""GPU: the grouped device parse (psg_mb_load_text_groups) against its host
twin (psg_text_parse_groups_host, itself held to tests/slot_ref.py on the CPU)
and against slot_ref, bit for bit: the CPU corpus, slot tokens and "\\r\\n"
ends across the kernels' lane (16 bytes) and chunk (psg_text_chunk()) edges,
slow slot tokens, more than 256 chunks, and the grouping that follows it."""
import numpy as np
import pytest

import slot_inputs
import slot_ref as S
from parameter_server_amd import _lib, slots
from parameter_server_amd.kv_vector import KVVector
from parameter_server_amd.worker import Minibatch, text_chunk

pytestmark = pytest.mark.gpu

CORPUS = slot_inputs.corpus()
NAMES = ("offset", "index", "value", "y", "slot")


@pytest.fixture(scope="module")
def mb():
    v = KVVector(0, _lib.PSG_F64)
    m = Minibatch(v._h)
    yield m
    m.close()
    v.close()


def bits(a):
    return None if a is None else np.ascontiguousarray(a).tobytes()


def check(mb, text, fmt, max_rows=None, final=True, ref=True):
    """Device == host twin (== slot_ref when `ref`), every array and count.
    slow_tokens: the device counts those of all the lines it took, the host
    stops at the rejected line, as for psg_mb_load_text."""
    host = slots.parse_text_groups_host(text, fmt, max_rows, final)
    r = mb.load_text_groups(text, fmt, max_rows, final)
    hr = host[5]
    assert (r.rows, r.nnz, r.consumed, r.bad_line) == (hr.rows, hr.nnz, hr.consumed, hr.bad_line)
    if hr.bad_line < 0:
        assert r.slow_tokens == hr.slow_tokens
    else:
        assert r.slow_tokens >= hr.slow_tokens
    got = {n: mb.read(n) for n in NAMES}
    for n, w in zip(NAMES, host[:5]):
        if w is None:
            assert got[n].size == 0
        else:
            assert bits(got[n]) == bits(w), n
    if ref:
        want = S.parse(text, fmt, max_rows, final)
        assert (r.rows, r.consumed, r.bad_line) == want[5:]
        for n, w in zip(NAMES, want[:5]):
            if w is not None:
                assert bits(got[n]) == bits(w), n
    return r, got


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_corpus(mb, name):
    check(mb, *CORPUS[name])


def at(prefix, lead, token_at):
    """`prefix` lines, then blanks, so that `lead`'s end is byte token_at."""
    pad = token_at - len(prefix) - len(lead)
    assert pad >= 0
    return prefix + b" " * pad + lead


def edges():
    c = text_chunk()
    return (48, 256, c, 2 * c)


@pytest.mark.parametrize("tok", (b"4095", b"+7", b"00007", b"\t7", b"0", b"4096"))
def test_slot_token_straddles_an_edge(mb, tok):
    first = b"a 1 1 5:1\n"
    for e in edges():
        for inside in range(1, len(tok)):  # bytes of the token before the edge
            text = at(first, b"b 1 0 77:", e - inside) + tok + b" 78:2\nc 1 1 9:3\n"
            assert text[e - inside:e - inside + len(tok)] == tok
            r, got = check(mb, text, S.ADFEA)
            assert r.bad_line == (1 if tok in (b"0", b"4096") else -1)


@pytest.mark.parametrize("end", (b"\r\n", b"\r\r\n", b" \r\n", b"\n"))
def test_line_end_straddles_an_edge(mb, end):
    first = b"a 1 1 5:1\n"
    for e in edges():
        for inside in range(0, len(end) + 1):  # bytes of the line end before the edge
            text = at(first, b"b 1 0 77:12", e - inside) + end + b"c 1 1 9:3 10:4\n"
            assert text[e - inside:e - inside + len(end)] == end
            r, got = check(mb, text, S.ADFEA)
            assert r.bad_line == (1 if end == b"\r\r\n" else -1)
            if r.bad_line < 0:
                assert got["slot"].tolist() == [1, 12, 3, 4]
    c = text_chunk()
    # '\r' the last byte of a chunk and '\n' the first of the next; and a text
    # that ends with its chunk in a '\r', final and not
    text = at(first, b"b 1 0 77:12\r", c) + b"\nc 1 1 9:3\n"
    assert text[c - 1:c + 1] == b"\r\n"
    check(mb, text, S.ADFEA)
    text = at(first, b"b 1 0 77:12\r", c)
    assert len(text) == c
    assert check(mb, text, S.ADFEA, final=True)[0].rows == 2
    assert check(mb, text, S.ADFEA, final=False)[0].rows == 1
    assert check(mb, text + b"\r", S.ADFEA, final=True)[0].bad_line == 1  # "12\r" then '\r'


def grouped_line(i, nf, slow=0.0, rng=None):
    """A fast-grammar line of nf entries in up to three groups; a share `slow`
    of its slot tokens written outside the fast grammar, same ids."""
    ent = []
    for j in range(nf):
        s = (1, 300, 4095)[min(3 * j // max(nf, 1), 2)] if i % 4 else 7
        k = (i * 1000003 + j * 7919) % (1 << 40)
        form = "%d" % s
        if rng is not None and rng.random() < slow:
            form = ("+%d" % s) if j % 2 else ("%05d" % s)
        ent.append("%d:%s" % (k, form))
    return ("r%d 1 %d %s%s" % (i, i % 2, " ".join(ent), "\r\n" if i % 3 == 0 else "\n")).encode()


def test_results_do_not_depend_on_the_slow_share(mb):
    texts = []
    for share in (0.0, 0.5, 1.0):
        rng = np.random.default_rng(4)
        texts.append(b"".join(grouped_line(i, 1 + i % 9, share, rng) for i in range(400)))
    out = []
    for share, text in zip((0.0, 0.5, 1.0), texts):
        r, got = check(mb, text, S.ADFEA)
        assert r.bad_line == -1 and r.rows == 400
        assert (r.slow_tokens == 0) == (share == 0.0)
        if share == 1.0:
            assert r.slow_tokens == r.nnz
        out.append(got)
    for n in NAMES:
        assert bits(out[0][n]) == bits(out[1][n]) == bits(out[2][n]), n


def test_slow_slot_in_the_first_and_the_last_line(mb):
    body = b"".join(grouped_line(i, 5) for i in range(1, 60))
    text = b"f 1 1 5:+2 6:2\n" + body + b"l 1 0 8:3 9:+3"
    r, got = check(mb, text, S.ADFEA)
    assert r.slow_tokens == 2 and r.rows == 61
    assert got["slot"][:2].tolist() == [2, 2] and got["slot"][-2:].tolist() == [3, 3]
    # ... and rejected there
    assert check(mb, b"f 1 1 5:-2\n" + body, S.ADFEA)[0].bad_line == 0
    assert check(mb, body + b"l 1 0 8:3 9:+0", S.ADFEA)[0].bad_line == 59


def test_more_than_256_chunks(mb):
    c = text_chunk()
    rng = np.random.default_rng(9)
    lines, size, i = [], 0, 0
    while size < 257 * c + c // 3:
        lines.append(grouped_line(i, 40 + i % 17, 0.01, rng))
        size += len(lines[-1])
        i += 1
    text = b"".join(lines)
    assert (len(text) + c - 1) // c > 256
    r, got = check(mb, text, S.ADFEA, ref=False)
    assert r.bad_line == -1 and r.rows == len(lines) and r.slow_tokens > 0
    # the grouping of what the device parsed, against slot_ref's bookkeeping
    info, bad = slots.mb_groups(mb)
    rows, skipped = S.skip_parse(text, S.ADFEA)
    assert bad == -1 and skipped == [] and info == S.info(rows, S.ADFEA)
    assert [s["id"] for s in info] == [0, 1, 7, 300, 4095]
    cut = len(lines) // 2
    assert check(mb, text, S.ADFEA, max_rows=cut, ref=False)[0].rows == cut


def test_groups_after_the_device_parse(mb):
    """The digits the grouping sorts on come from the device's own OR / AND of
    the slot ids: ids that differ in the low digit, the high digit, both, none."""
    for ids in ((1, 2), (1, 257), (2, 4095), (9, 9)):
        text = b"".join(b"r 1 1 %d:%d %d:%d %d:%d\n" % (3 * i, ids[0], 3 * i + 1, ids[1], 3 * i + 2,
                                                         ids[1]) for i in range(300))
        r = mb.load_text_groups(text, "adfea")
        info, bad = slots.mb_groups(mb)
        rows, _ = S.skip_parse(text, S.ADFEA)
        assert bad == -1 and info == S.info(rows, S.ADFEA)
    # LIBSVM: slot 1 on every line, empty ones included
    text = b"1 3:1.5 7:2\n-1\n0.5 2:0.25\r\n"
    mb.load_text_groups(text, "libsvm")
    assert mb.read("slot").tolist() == [1, 1, 1]
    info, bad = slots.mb_groups(mb)
    assert info == S.info(S.skip_parse(text, S.LIBSVM)[0], S.LIBSVM) and info[1]["nnz_ex"] == 3
    # a split id found after the device parse
    mb.load_text_groups(b"a 1 1 5:1\nb 1 1 5:2 6:9 7:2\n", "adfea")
    assert slots.mb_groups(mb) == ([], 1)
