"""CPU: the grouped host parse (psg_text_parse_groups_host) against
tests/slot_ref.py bit for bit over the corpus of tests/slot_inputs.py, the
feature blocks against the oracle's evenDivide, mergeExampleInfo, and the
skip bookkeeping of the Python layer through the host parse.  No device."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_py as O
import slot_inputs
import slot_ref as S
from parameter_server_amd import _lib, slots
from parameter_server_amd.worker import parse_text_host

CORPUS = slot_inputs.corpus()


def bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint8).tobytes()


def check_host(text, fmt, max_rows, final):
    want = S.parse(text, fmt, max_rows, final)
    offset, index, value, y, slot, r = slots.parse_text_groups_host(text, fmt, max_rows, final)
    assert (int(r.rows), int(r.consumed), int(r.bad_line)) == (want[5], want[6], want[7])
    assert int(r.nnz) == want[1].size
    assert bits(offset) == bits(want[0])
    assert bits(index) == bits(want[1])
    assert bits(value) == bits(want[2])
    assert bits(y) == bits(want[3])
    assert bits(slot) == bits(want[4])
    assert int(r.slow_tokens) == S.slow_tokens(text, fmt, max_rows, final)
    return want


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_host_parse_matches_reference(name):
    check_host(*CORPUS[name])


def test_corpus_reaches_what_it_names():
    """The corpus's lines do what their names say (so that a parser agreeing
    with a wrong restatement would still be noticed)."""
    p = lambda name: S.parse(*CORPUS[name])
    assert p("slot_ids")[4].tolist() == [1, 9, 10, 255, 256, 257, 4095, 4095, 257, 1]
    assert p("leading_zero_fast")[4].tolist() == [7, 7] and S.slow_tokens(*CORPUS["leading_zero_fast"]) == 0
    assert p("slow_accepted")[4].tolist() == [7, 7, 7] and S.slow_tokens(*CORPUS["slow_accepted"]) == 2
    assert p("tab_slot")[4].tolist() == [7, 7]
    assert p("wraps_to_1")[4].tolist() == [1, 1]
    for name in ("slot_0", "slot_4096", "slot_negative", "slot_junk", "slot_cr_then_token",
                 "crcrlf", "bad_middle"):
        two = CORPUS[name][0].index(b"\n", CORPUS[name][0].index(b"\n") + 1) + 1
        assert p(name)[5:] == (1, two, 1), name  # one row, two lines consumed, line 1 rejected
    assert p("crlf")[5:] == (2, len(CORPUS["crlf"][0]), -1) and p("crlf")[4].tolist() == [1, 2, 3]
    assert p("lone_cr_line_end")[7] == -1 and p("lone_cr_line_end")[1].tolist() == [5, 7]
    assert p("final_cr")[5] == 2 and p("final_cr")[4].tolist() == [1, 3]
    assert p("final_cr_not_final")[5] == 1
    assert p("no_entry")[0].tolist() == [0, 0, 1]
    assert p("dangling_key")[1].tolist() == [5, 7]
    assert p("bad_first")[5:] == (0, 10, 0)
    assert p("bad_last")[7] == 2
    assert p("max_rows")[5:] == (2, 20, -1)
    assert p("mixed_cr")[7] == 0


def test_libsvm_is_the_ungrouped_parse_with_slot_1():
    for name in ("libsvm", "libsvm_bad"):
        text, fmt, max_rows, final = CORPUS[name]
        a = slots.parse_text_groups_host(text, fmt, max_rows, final)
        b = parse_text_host(text, fmt, max_rows, final)
        for x, z in zip(a[:4], b[:4]):
            assert bits(x) == bits(z)
        assert a[4].tolist() == [1] * a[1].size
        for f in ("rows", "nnz", "consumed", "bad_line", "slow_tokens"):
            assert getattr(a[5], f) == getattr(b[4], f)


def test_sizes_call_and_short_arrays():
    L = _lib.lib()
    text = CORPUS["slot_ids"][0]
    r = _lib.TextResult()
    none = [None] * 5
    assert L.psg_text_parse_groups_host(text, len(text), 4, 1 << 62, 1, *none, 0, 0, C.byref(r)) == 0
    assert (r.rows, r.nnz) == (2, 10)
    offset, index, y = np.zeros(3, np.uint64), np.zeros(4, np.uint64), np.zeros(2)
    slot = np.zeros(4, np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.psg_text_parse_groups_host(text, len(text), 4, 1 << 62, 1, p(offset), p(index), None,
                                        p(y), p(slot), 2, 4, C.byref(r)) == _lib.PSG_ERR_SIZE
    assert slot.tolist() == [1, 9, 10, 255]
    assert L.psg_text_parse_groups_host(text, len(text), 4, 1 << 62, 1, p(offset), p(index), None,
                                        p(y), None, 2, 4, C.byref(r)) == _lib.PSG_ERR_ARG
    assert L.psg_text_parse_groups_host(text, len(text), 3, 1 << 62, 1, *none, 0, 0,
                                        C.byref(r)) == _lib.PSG_ERR_ARG


# ---- the Python layer's skip -------------------------------------------------------
SKIP_TEXT = (b"a 1 x 5:1\n"        # 0: rejected (label)
             b"b 1 1 5:1 6:2\n"
             b"c 1 1 5:0\n"        # 2: rejected (slot 0)
             b"d 1 0 7:2 8:9\r\n"
             b"e 1 1 9:4096\n"     # 4: rejected
             b"f 1 1\n"
             b"g 1")               # 6: rejected (no label), the final line


def test_skip_bad_has_no_effect_on_the_rest():
    offset, index, value, y, slot, bad = slots.parse_groups_skipping(SKIP_TEXT, "adfea")
    rows, want_bad = S.skip_parse(SKIP_TEXT, S.ADFEA)
    assert bad == want_bad == [0, 2, 4, 6]
    kept = b"".join(l for i, l in enumerate(SKIP_TEXT.splitlines(True)) if i not in bad)
    want = S.parse(kept, S.ADFEA)
    assert want[7] == -1 and want[5] == len(rows) == 3
    for got, w in zip((offset, index, value, y, slot), want[:5]):
        assert bits(got) == bits(w)


def test_skip_bad_false_raises_with_the_line_number():
    with pytest.raises(_lib.PSGError, match="line 0 of the text") as e:
        slots.parse_groups_skipping(SKIP_TEXT, "adfea", skip_bad=False)
    assert e.value.status == _lib.PSG_ERR_ARG
    clean = b"b 1 1 5:1 6:2\n"
    assert slots.parse_groups_skipping(clean, "adfea", skip_bad=False)[5] == []


def test_skip_not_final_leaves_the_partial_line():
    got = slots.parse_groups_skipping(b"a 1 1 5:1\nb 1 1 5:2", "adfea", final=False)
    assert got[3].size == 1 and got[5] == []


# ---- ExampleInfo -------------------------------------------------------------------
def slot(i, fmt, lo, hi, ele, ex):
    return {"id": i, "format": fmt, "min_key": lo, "max_key": hi, "nnz_ele": ele, "nnz_ex": ex}


def test_merge_example_info():
    a = {"num_ex": 10, "slot": [slot(0, 1, 0, 1, 10, 10), slot(3, 3, 5, 90, 40, 9)]}
    b = {"num_ex": 4, "slot": [slot(0, 1, 0, 1, 4, 4), slot(2, 3, 7, 8, 1, 1),
                               slot(3, 3, 2, 50, 8, 4)]}
    m = slots.merge_example_info(a, b)
    assert m == {"num_ex": 14, "slot": [slot(0, 1, 0, 1, 14, 14), slot(2, 3, 7, 8, 1, 1),
                                        slot(3, 3, 2, 90, 48, 13)]}
    assert a["slot"][1]["nnz_ele"] == 40  # the arguments are not changed
    assert slots.merge_example_info({"num_ex": 0, "slot": []}, b) == b
    with pytest.raises(ValueError):
        slots.merge_example_info(a, {"num_ex": 1, "slot": [slot(3, 2, 0, 1, 1, 1)]})


def ref_blocks(info, ratio):
    """batch_solver.cc:48-66 over the oracle's Range::evenDivide."""
    out = []
    for s in info:
        if s["id"] == 0:
            continue
        per_row = float(s["nnz_ele"]) / float(s["nnz_ex"])
        n = max(int(math.ceil(per_row * ratio)), 1) if per_row > 1 + 1e-6 else 1
        for i in range(n):
            b, e = O.even_divide(s["min_key"], s["max_key"], n, i)
            if b < e:
                out.append((s["id"], b, e))
    return out


@pytest.mark.parametrize("ratio", [0.0, 0.5, 1.0, 4.0])
def test_feature_blocks(ratio):
    info = [slot(0, 1, 0, 1, 100, 100),
            slot(1, 3, 10, 1000, 100, 100),            # nnz_per_row exactly 1: one block
            slot(2, 3, 10, 1000, 1000001, 1000000),    # 1 + 1e-6 exactly is not "over"
            slot(3, 3, 10, 1000, 1000002, 1000000),    # just over 1
            slot(4, 3, 0, (1 << 64) - 1, 700, 100),
            slot(5, 3, 7, 9, 900, 100),                # more blocks than keys: empty ones
            slot(6, 3, (1 << 63) - 5, (1 << 63) + 12345, 333, 100)]
    got = slots.feature_blocks(info, ratio)
    assert got == ref_blocks(info, ratio)
    assert slots.feature_blocks({"num_ex": 100, "slot": info}, ratio) == got
    assert all(g != 0 and kb < ke for g, kb, ke in got)
    assert [b for b in got if b[0] in (1, 2)] == [(1, 10, 1000), (2, 10, 1000)]
    if ratio == 4.0:
        assert len([b for b in got if b[0] == 5]) == 2 < math.ceil(9 * ratio)
        assert len([b for b in got if b[0] == 3]) == 5


def test_even_divide_entry():
    L = _lib.lib()
    for b, e, n in [(0, 0, 3), (5, 6, 4), (0, (1 << 64) - 1, 7), (123, 1 << 63, 1000)]:
        got = slots.even_divide(b, e, n)
        for i in range(n):
            assert (int(got[i]), int(got[i + 1])) == O.even_divide(b, e, n, i)
    out = np.zeros(2, np.uint64)
    p = out.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.psg_even_divide(0, 1, 0, p) == _lib.PSG_ERR_ARG
    assert L.psg_even_divide(2, 1, 1, p) == _lib.PSG_ERR_ARG
