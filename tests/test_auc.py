"""CPU: the two forms of tests/auc_ref.py agree bit for bit, hand-worked
answers, and the library's pure host functions psg_auc_accuracy_data /
psg_auc_evaluate_data against the restatement (no device calls).  The
restatement is pinned to the reference's compiled auc.h / evaluation.h in
tests/test_reference_pin.py; evaluate by key (PSG_AUC_BY_KEY) and exact-AUC
ties across the classes have no reference and are held here alone."""
import ctypes as C
import math

import numpy as np
import pytest

import auc_ref as R
from parameter_server_amd import _lib
from parameter_server_amd.auc import accuracy_data, evaluate_data

TILE = 2048  # the cases are the GPU tests' cases at the shipped sort tile
I64, U64 = np.int64, np.uint64


def fbits(v):
    """A double's bits; every NaN is one value (0 / 0 has no payload to keep)."""
    return "nan" if math.isnan(v) else int(R.bits(np.float64(v))[0])


ADD = R.add_cases(TILE)
EXACT = R.exact_cases(TILE)


def data_cases():
    """name -> (AUCData, goodness) for accuracy and evaluate."""
    out = {}
    for name in ("mixed_3Tp5_g10", "mixed_Tp1_g100000", "distinct", "one_key", "seam_run",
                 "mixed_1_g1"):
        y, p, g = ADD[name]
        out[name] = (R.vector_compute(y, p, g), g)
    big = 1 << 40
    out["counts_2p40"] = ((np.array([-3, 0, 7], I64), np.array([big, 3, big + 1], U64),
                           np.array([-3, 1, 9], I64), np.array([5, big, 2 * big + 3], U64)), 10)
    edge = (1 << 53) + 1  # (double)key rounds: 2^53 + 1 -> 2^53
    out["keys_past_2p53"] = ((np.array([-edge - 2, -edge, edge, edge + 2], I64),
                              np.array([1, 2, 3, 4], U64),
                              np.array([R.INT64_MIN, -edge, edge, (1 << 63) - 1], I64),
                              np.array([4, 3, 2, 1], U64)), 1 << 53)
    z64, zu = np.zeros(0, I64), np.zeros(0, U64)
    out["no_negatives"] = ((np.array([1, 2], I64), np.array([3, 4], U64), z64, zu), 10)
    out["no_positives"] = ((z64, zu, np.array([1, 2], I64), np.array([3, 4], U64)), 10)
    out["empty"] = ((z64, zu, z64, zu), 10)
    return out


DATA = data_cases()
THRESHOLDS = (0.0, 0.5, -0.5, 1.0 + 2.0 ** -52)


@pytest.mark.parametrize("name", sorted(ADD))
def test_compute_forms_agree(name):
    y, p, g = ADD[name]
    a, b = R.scalar_compute(y, p, g), R.vector_compute(y, p, g)
    assert R.same_data(a, b)
    assert int(a[1].sum()) + int(a[3].sum()) == y.size


def test_key_rule():
    assert R.scalar_key(0.4, 10) == 4 and R.scalar_key(-0.4, 10) == -4
    assert R.scalar_key(0.4, 1) == 0 and R.scalar_key(-0.4, 1) == 0  # toward zero, both sides
    for p in (math.nan, math.inf, -math.inf, 2.0 ** 63, -2.0 ** 63, 1e300):
        assert R.scalar_key(p, 1) == R.INT64_MIN
    assert R.scalar_key(2.0 ** 62, 1) == 1 << 62
    assert R.scalar_key(math.nextafter(2.0 ** 63, 0), 1) == (1 << 63) - 1024
    k = R.vector_keys(np.array([0.4, -0.4, math.nan, 2.0 ** 63, -9.3e18, 2.0 ** 62]), 1)
    assert k.tolist() == [0, 0, R.INT64_MIN, R.INT64_MIN, R.INT64_MIN, 1 << 62]


def test_merge_forms_agree_and_equal_one_compute():
    y, p, g = ADD["mixed_3Tp5_g10"]
    cuts = [0, 100, 100, TILE + 3, 2 * TILE, y.size]
    parts = [R.vector_compute(y[a:b], p[a:b], g) for a, b in zip(cuts, cuts[1:])]
    rng = np.random.default_rng(5)
    shuffled = []
    for tk, tc, fk, fc in parts:  # unsorted lists, a repeat and a zero count
        o, q = rng.permutation(tk.size), rng.permutation(fk.size)
        shuffled.append((np.concatenate([tk[o], tk[:1], [12345]]).astype(I64),
                         np.concatenate([tc[o] - (np.arange(tk.size) == 0)[o].astype(U64),
                                         np.ones(min(1, tk.size), U64), [0]]).astype(U64),
                         fk[q], fc[q]))
    a, b = R.scalar_merge(shuffled), R.vector_merge(shuffled)
    assert R.same_data(a, b)
    assert R.same_data(a, R.vector_compute(y, p, g))
    assert 12345 not in a[0].tolist()


@pytest.mark.parametrize("name", sorted(DATA))
def test_accuracy_and_evaluate_forms_agree_and_the_library_matches(name):
    data, g = DATA[name]
    for th in THRESHOLDS:
        want = R.scalar_accuracy(data, g, th)
        assert fbits(want) == fbits(R.vector_accuracy(data, g, th))
        assert fbits(want) == fbits(accuracy_data(g, *data, threshold=th))
    for as_written in (False, True):
        want = R.scalar_evaluate(data, as_written)
        assert fbits(want) == fbits(R.vector_evaluate(data, as_written))
        assert fbits(want) == fbits(evaluate_data(*data, as_written=as_written))


def test_hand_worked():
    # 3 positives at keys {1, 3, 5}, 2 negatives at {2, 4}, every count 1: by
    # key the negatives have 1 and 2 positives at or below them, so
    # (1 + 2) / 3 / 2 = 0.5, which is not < .5 and stays
    data = (np.array([1, 3, 5], I64), np.ones(3, U64), np.array([2, 4], I64), np.ones(2, U64))
    by_key = (1.0 * 1 + 2.0 * 1) / 3.0 / 2.0
    assert R.scalar_evaluate(data) == (1 - by_key if by_key < .5 else by_key) == 0.5
    # as written: every count is 1 <= 1, so the first negative takes all three
    # positives: (3 + 3) / 3 / 2 = 1.0 whatever the keys
    assert R.scalar_evaluate(data, as_written=True) == 1.0
    assert evaluate_data(*data) == 0.5 and evaluate_data(*data, as_written=True) == 1.0
    # positives at {2, 4, 5}, negatives at {1, 3}: 0 and 1 positives at or
    # below -> 1/6 -> 1 - 1/6 = 5/6; as written still 1.0
    data = (np.array([2, 4, 5], I64), np.ones(3, U64), np.array([1, 3], I64), np.ones(2, U64))
    want = 1 - (0.0 + 1.0) / 3.0 / 2.0
    assert R.scalar_evaluate(data) == want == evaluate_data(*data)
    assert abs(want - 5 / 6) < 1e-15
    assert evaluate_data(*data, as_written=True) == 1.0
    # accuracy at goodness 10, threshold 0.25 -> x = 2.5: positives at 4, 5
    # and the negative at 1 are right: 3 / 5
    assert accuracy_data(10, *data, threshold=0.25) == 3.0 / 5.0 == R.scalar_accuracy(data, 10, .25)
    # (double)key rounds in the compare: key 2^53 + 1 against x = 2^53 + 2
    edge = (np.array([(1 << 53) + 1], I64), np.ones(1, U64), np.zeros(0, I64), np.zeros(0, U64))
    assert accuracy_data(1, *edge, threshold=float((1 << 53) + 2)) == 0.0
    assert accuracy_data(1, *edge, threshold=float(1 << 53)) == 1.0  # 2^53 + 1 -> 2^53 >= 2^53
    empty = (np.zeros(0, I64), np.zeros(0, U64), np.zeros(0, I64), np.zeros(0, U64))
    assert math.isnan(accuracy_data(10, *empty)) and evaluate_data(*empty) == 0.5


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_forms_agree(name):
    y, p = EXACT[name]
    a, b = R.scalar_exact(y, p), R.vector_exact(y, p)
    assert fbits(a) == fbits(b)
    if name.startswith("all_"):
        assert math.isnan(a)


def test_exact_hand_worked():
    # the two zeros are one value: input order decides, not the sign
    assert R.scalar_exact([1.0, -1.0], [-0.0, 0.0]) == 1.0  # positive first: 1 / (1 * 1)
    assert R.scalar_exact([1.0, -1.0], [0.0, -0.0]) == 1.0
    assert R.scalar_exact([-1.0, 1.0], [-0.0, 0.0]) == 1.0  # 0 -> 1 - 0
    # predictions 1..4, positives at 2 and 4: negatives see 0 and 1 -> 1/4 -> 3/4
    assert R.scalar_exact([-1, 1, -1, 1], [1.0, 2.0, 3.0, 4.0]) == 0.75
    assert R.vector_exact([-1, 1, 0.0, np.nan, 1], [1.0, 2.0, 3.0, 3.5, 4.0]) == 1 - 2 / 6


def test_bad_arguments_need_no_device():
    L = _lib.lib()
    one, cnt = np.zeros(1, I64), np.ones(1, U64)
    out = np.zeros(1)
    assert L.psg_auc_evaluate_data(one.ctypes.data, cnt.ctypes.data, 1, one.ctypes.data,
                                   cnt.ctypes.data, 1, 7,
                                   out.ctypes.data_as(C.POINTER(C.c_double))) == _lib.PSG_ERR_ARG
    assert L.psg_auc_accuracy_data(1, None, None, 1, None, None, 0, 0.0, None) == _lib.PSG_ERR_ARG
    with pytest.raises(_lib.PSGError):
        evaluate_data(one, np.ones(2, U64), one, cnt)


def test_the_sort_shape_of_psg_auc_is_the_workers():
    """psg_sort.h defines the shape its kernels are built to, once; psg_auc.hip
    and psg_worker.hip include it and define none of it, so the GPU tests,
    which size their cases by psg_mb_sort_tile(), size them for both."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "parameter_server_amd", "csrc")
    sort, worker, mine = (open(os.path.join(csrc, f)).read()
                          for f in ("psg_sort.h", "psg_worker.hip", "psg_auc.hip"))
    for name in ("PSG_SORT_KPT", "kSortKPT", "kSortTile", "kWaveSpan", "kFlagTile"):
        pat = r"^\s*(?:#\s*define\s+%s\b|(?:static\s+)?(?:constexpr|const)\b[^;=]*\b%s\s*=)" % (
            name, name)
        assert len(re.findall(pat, sort, flags=re.M)) == 1, name
        for src in (worker, mine):
            assert not re.findall(pat, src, flags=re.M), name
    for src in (worker, mine):
        assert len(re.findall(r'^#include "psg_sort.h"', src, flags=re.M)) == 1
