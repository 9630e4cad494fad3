"""CPU: the TERAFEA host parse (psg_text_parse_terafea_host) against the plain
restatement tests/terafea_ref.py on the inputs of terafea_ref.cases, exactly,
and the ABI's bad arguments."""
import ctypes as C

import numpy as np
import pytest

import terafea_ref as R
from parameter_server_amd import _lib, slots
from parameter_server_amd.worker import terafea_tile, text_chunk

CASES = R.cases(terafea_tile(), text_chunk())
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def same(got, want):
    """offset, index, y, slot, then rows, nnz, consumed, bad_line: all exact."""
    for g, w in zip(got[:4], want[:4]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert tuple(got[4:]) == tuple(want[4:])


@pytest.mark.parametrize("shuffle,beta", FLAGS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_parse_matches_restatement(name, shuffle, beta):
    text, max_rows, final = CASES[name]
    offset, index, _, y, slot, r = slots.parse_text_groups_host(text, "terafea", max_rows, final,
                                                                shuffle, beta)
    same((offset, index, y, slot, r.rows, r.nnz, r.consumed, r.bad_line),
         R.parse(text, shuffle, beta, max_rows, final))


def test_slow_tokens_are_counted():
    L = _lib.lib()
    r = _lib.TextResult()
    text = CASES["slow"][0]
    _lib.check(L.psg_text_parse_terafea_host(text, len(text), 0, 1 << 40, 1, None, None, None,
                                             None, 0, 0, C.byref(r)))
    assert r.slow_tokens == 4  # "+key", 21 digits, "\tkey", label "+1"


def test_bad_arguments():
    L = _lib.lib()
    r = _lib.TextResult()
    t = b"1 id | %d\n" % R.G
    assert L.psg_text_parse_terafea_host(t, len(t), 4, 9, 1, None, None, None, None, 0, 0,
                                         C.byref(r)) == _lib.PSG_ERR_ARG
    assert L.psg_text_parse_terafea_host(t, len(t), 0, 9, 1, None, None, None, None, 0, 0,
                                         None) == _lib.PSG_ERR_ARG
    off = np.zeros(2, np.uint64)
    p = off.ctypes.data_as(C.c_void_p)
    assert L.psg_text_parse_terafea_host(t, len(t), 0, 9, 1, p, None, None, None, 1, 1,
                                         C.byref(r)) == _lib.PSG_ERR_ARG
    y, idx, slot = np.zeros(1), np.zeros(1, np.uint64), np.zeros(1, np.uint16)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.psg_text_parse_terafea_host(t, len(t), 0, 9, 1, p, ptr(idx), ptr(y), ptr(slot), 0,
                                         0, C.byref(r)) == _lib.PSG_ERR_SIZE
