"""GPU: psg_mb_load_text (parameter_server_amd/csrc/psg_text.hip) at its lane,
wave and scan edges, on the inputs of text_inputs (whose structure
test_text_inputs.py proves on the CPU): more than one chunk per lane of the
chunk scan, the carry between the waves of a chunk, dense lanes, the text's
end, two rejected lines, the order search over equal offsets, max_rows cuts
and the fast converters as the device compiles them.  Every load goes through
test_text_gpu.check: rows, nnz, consumed, bad_line, slow_tokens and the
arrays against text_ref.parse, bit for bit, on one handle for the module."""
import ctypes as C

import pytest

import text_inputs as I
from test_text_gpu import check
from parameter_server_amd import _lib
from parameter_server_amd.worker import Minibatch

pytestmark = pytest.mark.gpu
FORMATS = I.FORMATS


@pytest.fixture(scope="module")
def mb():
    """One context and one handle for every case: sizes from 0 bytes to 516
    chunks follow each other on the same blocks."""
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    m = Minibatch(h)
    yield m
    m.close()
    L.psg_destroy(h)


def load(mb, case):
    return check(mb, case.text, case.fmt, case.max_rows, case.final)[0]


def walk_on(mb, text, fmt, at):
    """The loads that follow the one that consumed `at` bytes: (rows, bad_line) each."""
    out = []
    while at < len(text):
        r, _ = check(mb, text[at:], fmt)
        assert r.consumed > 0
        at += r.consumed
        out.append((r.rows, r.bad_line))
    return out


@pytest.mark.parametrize("variant", ["plain", "cut", "bad"])
@pytest.mark.parametrize("nc", I.MANY_CHUNKS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_many_chunks(mb, fmt, nc, variant):
    case = {x.name: x for x in I.many_chunks(fmt, nc)}[variant]
    k = case.claims
    r = load(mb, case)
    assert r.slow_tokens >= 3
    if variant == "plain":
        assert (r.rows, r.bad_line, r.consumed) == (k["rows"], -1, len(case.text))
    elif variant == "cut":
        assert (r.rows, r.bad_line, r.consumed) == (case.max_rows, -1, k["consumed"])
    else:
        assert (r.rows, r.bad_line, r.consumed) == (k["bad"], k["bad"], k["consumed"])
        assert walk_on(mb, case.text, fmt, r.consumed) == [(k["rows"] - k["bad"] - 1, -1)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_wave_gaps(mb, fmt):
    for case in I.wave_gaps(fmt):
        r = load(mb, case)
        assert (r.rows, r.bad_line) == (case.claims["rows"], -1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_lane_dense(mb, fmt):
    for case in I.lane_dense(fmt):
        r = load(mb, case)
        assert r.bad_line == case.claims.get("bad", -1) and r.slow_tokens >= 1
        if r.bad_line >= 0:
            assert all(bad == -1 for _, bad in walk_on(mb, case.text, fmt, r.consumed))


@pytest.mark.parametrize("fmt", FORMATS)
def test_text_ends(mb, fmt):
    for case in I.text_ends(fmt):
        r = load(mb, case)
        assert (r.rows, r.bad_line) == (case.claims["rows"], -1)


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_bad(mb, fmt):
    for case in I.two_bad(fmt):
        k = case.claims
        r = load(mb, case)
        assert (r.rows, r.bad_line, r.consumed) == (k["bad"], k["bad"], k["consumed"]), case.name
        rest = walk_on(mb, case.text, fmt, r.consumed)
        n = k["bad2"] - k["bad"] - 1
        assert rest == [(n, n), (k["rows"] - k["bad2"] - 1, -1)], case.name


def test_order_edges(mb):
    for case in I.order_edges():
        r = load(mb, case)
        assert r.bad_line == case.claims["bad"], case.name
        if r.bad_line >= 0:
            assert all(bad == -1 for _, bad in walk_on(mb, case.text, case.fmt, r.consumed))


@pytest.mark.parametrize("fmt", FORMATS)
def test_row_cuts(mb, fmt):
    for case in I.row_cuts(fmt):
        r = load(mb, case)
        assert (r.rows, r.consumed, r.bad_line) == (case.claims["rows"], case.claims["cut"], -1), case.name


@pytest.mark.parametrize("fmt", FORMATS)
def test_converter_sweep(mb, fmt):
    for case in I.converter_sweep(fmt):
        k = case.claims
        r = load(mb, case)
        assert (r.rows, r.bad_line, r.slow_tokens) == (k["rows"], -1, k["slow"])
        assert r.nnz == 2 * k["rows"]
