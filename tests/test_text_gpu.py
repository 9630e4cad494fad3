"""GPU: psg_mb_load_text (parameter_server_amd/csrc/psg_text.hip) against the
restatement of the reference's reader (tests/text_ref.py), bit for bit: the
arrays psg_mb_read gives back after a load from text, rows, nnz, consumed and
bad_line, with tokens, newlines and ':' placed around the kernels' chunk
boundaries, and the worker step from text against the step from arrays."""
import ctypes as C

import numpy as np
import pytest

import text_ref as T
from test_text import ADFEA_LINES, LIBSVM_LINES, bits, corpus
from parameter_server_amd import _lib
from parameter_server_amd.ftrl import FTRLModel
from parameter_server_amd.worker import FTRLWorker, Minibatch, text_chunk

pytestmark = pytest.mark.gpu
FORMATS = (T.LIBSVM, T.ADFEA)


@pytest.fixture(scope="module")
def ctx():
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    yield h
    L.psg_destroy(h)


@pytest.fixture(scope="module")
def mb(ctx):
    """One handle for the whole module: every test also tests reuse."""
    m = Minibatch(ctx)
    yield m
    m.close()


def arrays(mb):
    return mb.read("offset"), mb.read("index"), mb.read("value"), mb.read("y")


def same_arrays(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(bits(got[2]), bits(want[2]))
            and np.array_equal(bits(got[3]), bits(want[3])))


def check(mb, text, fmt, max_rows=None, final=True):
    """load_text == the restatement; returns (result, arrays)."""
    offset, index, value, y, rows, consumed, bad = T.parse(text, fmt, max_rows, final)
    if value is None:
        value = np.zeros(0, np.float64)
    r = mb.load_text(text, fmt, max_rows, final)
    what = (text[:60], len(text), fmt, max_rows, final)
    assert (r.rows, r.nnz, r.consumed, r.bad_line) == (rows, index.size, consumed, bad), what
    got = arrays(mb)
    assert np.array_equal(got[0], offset), what
    assert np.array_equal(got[1], index), what
    assert np.array_equal(bits(got[2]), bits(value)), what
    assert np.array_equal(bits(got[3]), bits(y)), what
    assert r.slow_tokens == T.slow_tokens(text, fmt, max_rows, final), what
    # the tail is psg_mb_load's: the row of every position
    assert np.array_equal(mb.read("row_of"),
                          np.repeat(np.arange(rows, dtype=np.uint32), np.diff(offset).astype(np.int64)))
    return r, got


def line(fmt, i, nf=1):
    """A line of nf entries whose numbers are all in the fast grammar."""
    keys = [(i * 1000003 + j + 1) * 1844674407370955 % (1 << 64) for j in range(nf)]
    keys.sort()
    if fmt == T.LIBSVM:
        return ("%d " % (i % 3 - 1) + " ".join("%d:%d.%06d" % (k, j % 7, (k >> 7) % 1000000)
                                               for j, k in enumerate(keys)) + "\n").encode()
    return ("%d 1 %d " % (i, i % 2) + " ".join("%d:%d" % (k, j) for j, k in enumerate(keys))
            + "\n").encode()


def placed(fmt, lines, target, within, at):
    """The lines as one text, line 0 padded with blanks so that byte `within`
    of line `target` (> 0) falls at place `at`."""
    pos = sum(len(l) for l in lines[:target]) + within
    assert pos <= at
    first = lines[0]
    cut = first.index(b" ") + 1
    text = first[:cut] + b" " * (at - pos) + first[cut:] + b"".join(lines[1:])
    assert text[at] == lines[target][within]
    return text


@pytest.mark.parametrize("fmt", FORMATS)
def test_chunk_boundaries(mb, fmt):
    c = text_chunk()
    lines = [line(fmt, i, 1 + i % 3) for i in range(4 * c // 30)]
    assert sum(map(len, lines)) > 3 * c
    t = len(lines) // 2
    tl = lines[t]
    key_at = tl.index(b" ", tl.index(b" ", tl.index(b" ") + 1) + 1) + 1 if fmt == T.ADFEA \
        else tl.index(b" ") + 1
    colon = tl.index(b":")
    base = sum(map(len, lines[:t]))
    k = (base + len(tl) + c - 1) // c + 1  # a boundary all of these can be pushed to
    for within in (key_at + 5, key_at, key_at + 1,      # a token straddles; starts at; one before
                   len(tl) - 1, len(tl),                # '\n' first byte of a chunk; last byte
                   colon, colon + 1):                   # ':' first byte of a chunk; last byte
        if within == len(tl):
            text = placed(fmt, lines, t + 1, 0, k * c)
            assert text[k * c - 1:k * c] == b"\n"
        else:
            text = placed(fmt, lines, t, within, k * c)
        r, _ = check(mb, text, fmt)
        assert r.bad_line == -1 and r.rows == len(lines) and r.slow_tokens == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_long_line_and_chunk_without_newline(mb, fmt):
    c = text_chunk()
    nf = 3 * c // 28
    long_line = line(fmt, 5, nf)
    assert 2 * c + 64 < len(long_line) < 60 * 1024
    lines = [line(fmt, i) for i in range(40)] + [long_line] + [line(fmt, i) for i in range(50, 90)]
    text = placed(fmt, lines, 40, 0, c - 16)  # it covers all of chunk 1 and of chunk 2
    assert b"\n" not in text[c:3 * c]
    r, _ = check(mb, text, fmt)
    assert r.rows == 81 and r.nnz == 80 + nf
    r, _ = check(mb, long_line, fmt)  # alone: the first chunks hold no newline at all
    assert r.rows == 1


@pytest.mark.parametrize("fmt", FORMATS)
def test_small_texts(mb, fmt):
    one = line(fmt, 1, 3)
    assert check(mb, one, fmt)[0].rows == 1
    assert check(mb, b"", fmt)[0].consumed == 0
    assert check(mb, b"", fmt, final=False)[0].rows == 0
    assert check(mb, one * 7, fmt)[0].rows == 7  # shorter than one chunk
    for final in (True, False):  # no trailing newline
        r, _ = check(mb, one * 7 + one[:-1], fmt, final=final)
        assert r.rows == (8 if final else 7)
        r, _ = check(mb, one[:-1], fmt, final=final)
        assert r.rows == (1 if final else 0)
    if fmt == T.LIBSVM:  # all rows label-only
        r, _ = check(mb, b"1\n-1\n0.5\n" * 700, fmt)
        assert (r.rows, r.nnz) == (2100, 0)
    else:  # an ADFEA row without entries can only end the data
        r, _ = check(mb, b"a b 1", fmt)
        assert (r.rows, r.nnz) == (1, 0)
    check(mb, one * 7, fmt, max_rows=0)


@pytest.mark.parametrize("fmt", FORMATS)
def test_max_rows_and_rejected_line_in_chunk_2(mb, fmt):
    c = text_chunk()
    lines = [line(fmt, i, 2) for i in range(4 * c // 40)]
    at, cut = 0, None
    for i, l in enumerate(lines):
        at += len(l)
        if at > c + c // 2:
            cut = i  # the line that ends in the middle of chunk 2 (the second chunk)
            break
    text = b"".join(lines)
    r, _ = check(mb, text, fmt, max_rows=cut + 1)
    assert r.rows == cut + 1 and c < r.consumed < 2 * c
    for bad in (b"1 5:1 4:1\n" if fmt == T.LIBSVM else b"a b 1 5:1 4\n",   # by the order / by libc
                b"1 5:1 4\n" if fmt == T.LIBSVM else b"a b\n",              # on sight
                b"1 5:1 4:1\0\n" if fmt == T.LIBSVM else b"a b 1 5:1\0\n"):
        text = b"".join(lines[:cut] + [bad] + lines[cut:])
        r, _ = check(mb, text, fmt)
        assert (r.rows, r.bad_line) == (cut, cut) and r.consumed == at - len(lines[cut]) + len(bad)
        rest, _ = check(mb, text[r.consumed:], fmt)
        assert rest.rows == len(lines) - cut and rest.bad_line == -1
        check(mb, text, fmt, max_rows=cut)      # the rejected line is not reached
        check(mb, text, fmt, max_rows=cut + 1)


def test_quirks_as_one_text(mb):
    for fmt, lines in ((T.LIBSVM, LIBSVM_LINES), (T.ADFEA, ADFEA_LINES)):
        text = b"".join(l if l.endswith(b"\n") else l + b"\n" for l in lines)
        at, slow = 0, 0
        while at < len(text):
            r, _ = check(mb, text[at:], fmt)
            assert r.consumed > 0
            at += r.consumed
            slow += r.slow_tokens
        assert slow > 0
        assert mb.load_text(text, fmt).slow_tokens == T.slow_tokens(text, fmt) > 0


def test_every_token_slow(mb):
    rng = np.random.default_rng(3)
    for fmt in FORMATS:
        out, tokens = [], 0
        for r in range(600):
            keys = np.sort(rng.integers(0, 1 << 62, 1 + r % 5, dtype=np.uint64))
            if fmt == T.LIBSVM:
                out.append("%de0 " % (r % 2) + " ".join("%d:%.4e" % (k, rng.normal()) for k in keys))
            else:
                out.append("%d 1 +%d " % (r, r % 2) + " ".join("+%d:%d" % (k, r) for k in keys))
            tokens += 1 + keys.size
        text = ("\n".join(out) + "\n").encode()
        assert len(text) > 3 * text_chunk()
        r, _ = check(mb, text, fmt)
        assert r.slow_tokens == tokens and r.bad_line == -1


@pytest.mark.parametrize("fmt", FORMATS)
def test_reuse_and_interleaving(ctx, mb, fmt):
    large, small = corpus(fmt, 1500, seed=5), corpus(fmt, 20, seed=6)
    _, a = check(mb, large, fmt)
    check(mb, small, fmt)
    _, b = check(mb, large, fmt)
    assert same_arrays(a, b)
    # psg_mb_load in between, and a fresh handle: the same arrays all the way to the sort
    offset, index, value, y, _, _, _ = T.parse(small, fmt)
    mb.load(offset, index, value, y)
    assert same_arrays(arrays(mb), (offset, index, value if value is not None else np.zeros(0), y))
    mb.load_text(large, fmt)
    mb.uniq()
    fresh = Minibatch(ctx)
    fresh.load_text(large, fmt)
    fresh.uniq()
    assert same_arrays(arrays(mb), arrays(fresh)) and same_arrays(arrays(mb), a)
    for name in ("row_of", "sorted_key", "sorted_pos", "uniq_key", "key_cnt"):
        assert np.array_equal(mb.read(name), fresh.read(name)), name
    woffset, windex, wvalue, wy, _, _, _ = T.parse(large, fmt)
    fresh.load(woffset, windex, wvalue, wy)
    fresh.uniq()
    for name in ("row_of", "sorted_key", "sorted_pos", "uniq_key", "key_cnt"):
        assert np.array_equal(mb.read(name), fresh.read(name)), name
    fresh.close()


PARAM = dict(alpha=0.1, beta=1.0, lambda1=0.01, lambda2=0.1)


def workload(fmt, rows=900, seed=9):
    """Text whose keys repeat (Zipf), so the tail filter both drops and keeps."""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(rows):
        keys = np.unique(rng.zipf(1.3, 1 + int(rng.integers(1, 9))).astype(np.uint64) * 1000003)
        if fmt == T.LIBSVM:
            out.append("%d " % rng.choice((-1, 1)) + " ".join(
                "%d:%s" % (k, ("%.4f" % rng.normal()) if j % 4 else "%.3e" % rng.normal())
                for j, k in enumerate(keys)))
        else:
            out.append("%d 1 %d " % (r, rng.integers(0, 2)) + " ".join("%d:%d" % (k, j)
                                                                      for j, k in enumerate(keys)))
    return ("\n".join(out) + "\n").encode()


def make_worker():
    model = FTRLModel(0, capacity_hint=4096)
    model.setLearningRate(PARAM["alpha"], PARAM["beta"])
    model.setPenalty(PARAM["lambda1"], PARAM["lambda2"])
    return model, FTRLWorker(model, tail_feature_freq=2, countmin_n=1 << 16, countmin_k=2)


@pytest.mark.parametrize("fmt", FORMATS)
def test_step_text_end_to_end(fmt):
    text = workload(fmt)
    model_t, worker_t = make_worker()
    model_a, worker_a = make_worker()
    at = 0
    for b in range(3):
        objv_t, rows_t, consumed = worker_t.step_text(text[at:], fmt, max_rows=300)
        offset, index, value, y, rows, used, bad = T.parse(text[at:], fmt, max_rows=300)
        assert (rows_t, consumed, bad) == (300, used, -1)
        objv_a, rows_a = worker_a.step(offset, index, value, y)
        assert rows_a == rows_t and bits(np.float64(objv_t)) == bits(np.float64(objv_a))
        assert np.array_equal(worker_t.last_dict(), worker_a.last_dict())
        assert 0 < worker_t.ndict < worker_t.mb.n_uniq or b > 0
        at += consumed
    assert at == len(text)
    assert worker_t.num_ex == worker_a.num_ex == 900
    assert bits(np.float64(worker_t.objv)) == bits(np.float64(worker_a.objv))
    (kt, wt), (ka, wa) = model_t.export(), model_a.export()
    assert kt.size > 0 and np.array_equal(kt, ka) and np.array_equal(bits(wt), bits(wa))
    # predict_text against predict, on the trained models
    xw_t, consumed = worker_t.predict_text(text, fmt, max_rows=300)
    offset, index, value, y, _, used, _ = T.parse(text, fmt, max_rows=300)
    worker_a.predict(offset, index, value, y)
    assert consumed == used
    assert np.array_equal(bits(worker_t.mb.read("xw")), bits(worker_a.mb.read("xw")))
    assert np.any(worker_t.mb.read("xw") != 0)
    for w, m in ((worker_t, model_t), (worker_a, model_a)):
        w.close()
        m.close()
