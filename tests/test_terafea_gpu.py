"""GPU: psg_mb_load_terafea (the tokeniser's third form, the row sort's tile,
cut-row and long-row kernels, the finish) against its host twin and the plain
restatement tests/terafea_ref.py, every array and count exact, on the inputs
of terafea_ref.cases; then SlotReader from TERAFEA text."""
import numpy as np
import pytest

import terafea_ref as R
from parameter_server_amd import _lib, slots
from parameter_server_amd.kv_vector import KVVector
from parameter_server_amd.worker import Minibatch, terafea_tile, text_chunk

pytestmark = pytest.mark.gpu

CASES = R.cases(terafea_tile(), text_chunk())
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
SORT = ("lengths", "packing", "groups")  # where the flags change what the kernels do
PARAMS = [(n, s, b) for n in sorted(CASES) for s, b in (FLAGS if n in SORT else FLAGS[::3])]


@pytest.fixture(scope="module")
def ctx():
    v = KVVector(0, _lib.PSG_F64)
    yield v._h
    v.close()


@pytest.fixture(scope="module")
def mb(ctx):
    m = Minibatch(ctx)
    yield m
    m.close()


@pytest.mark.parametrize("name,shuffle,beta", PARAMS)
def test_device_load_matches_host_and_restatement(mb, name, shuffle, beta):
    text, max_rows, final = CASES[name]
    want = R.parse(text, shuffle, beta, max_rows, final)
    host = slots.parse_text_groups_host(text, "terafea", max_rows, final, shuffle, beta)
    r = mb.load_terafea(text, shuffle, beta, max_rows, final)
    assert (r.rows, r.nnz, r.consumed, r.bad_line) == tuple(want[4:])
    hr = host[5]  # the host stops counting at a rejected line
    assert r.slow_tokens == hr.slow_tokens if hr.bad_line < 0 else r.slow_tokens >= hr.slow_tokens
    if name == "slow":
        assert r.slow_tokens == 4
    for n, w, h in zip(("offset", "index", "y", "slot"), want[:4], (host[0], host[1], host[3],
                                                                    host[4])):
        got = mb.read(n)
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes() == h.tobytes(), n


def test_slot_reader_from_terafea(ctx):
    text = CASES["packing"][0] + CASES["groups"][0]
    offset, index, y, slot, rows = R.parse(text, shuffle=True)[:5]
    sr, dst = slots.SlotReader(ctx), Minibatch(ctx)
    try:
        assert sr.read(text, "terafea", shuffle=True) == R.info(offset, index, slot, rows)
        assert sr.example_info()["num_ex"] == rows and sr.bad_lines == []
        for g in (1023, int(slot[0])):
            sr.extract(g, dst)
            off_g, idx_g = R.group_matrix(offset, index, slot, g)
            assert dst.read("offset").tobytes() == off_g.tobytes()
            assert dst.read("index").tobytes() == idx_g.tobytes()
            assert dst.read("y").tobytes() == y.tobytes()
    finally:
        dst.close()
        sr.close()
