"""CPU: the two restatements of FTRLModel::setValue (tests/ftrl_ref.py) agree
bit for bit and take every branch; the library exports the psg_ftrl_* ABI and
the Python mirror imports (no device calls)."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import ftrl_ref as R
from parameter_server_amd import _lib

FTRL_SYMBOLS = ["psg_ftrl_init", "psg_ftrl_reserve", "psg_ftrl_push", "psg_ftrl_push_dev",
                "psg_ftrl_pull", "psg_ftrl_pull_dev", "psg_ftrl_status", "psg_ftrl_export",
                "psg_ftrl_lookup"]


def fbits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


NEG_ZERO = fbits(-0.0)


@pytest.fixture(scope="module")
def parity():
    uni, msgs = R.parity_case(seed=1)
    s, v = R.ScalarFTRL(**R.PARITY_PARAM), R.VectorFTRL(**R.PARITY_PARAM)
    states = []
    for m in msgs:
        s.push(*m)
        v.push(*m)
        states.append((s.lookup(uni), v.lookup(uni), s.nnz, v.nnz, s.entries, v.entries))
    return uni, msgs, s, v, states


def test_restatements_agree_on_the_parity_case(parity):
    uni, msgs, s, v, states = parity
    for a, b, nnz_s, nnz_v, ent_s, ent_v in states:
        for x, y in zip(a[:2], b[:2]):
            assert np.array_equal(x, y)
        assert np.array_equal(R.bits(a[2]), R.bits(b[2]))
        assert np.array_equal(R.bits(a[3]), R.bits(b[3]))
        assert np.array_equal(a[4], b[4])
        assert (nnz_s, ent_s) == (nnz_v, ent_v)
    assert s.transitions == v.transitions
    # nnz is the count of nonzero weights
    assert s.nnz == int(np.count_nonzero(s.lookup(uni)[2]))


def test_parity_case_takes_every_bookkeeping_branch(parity):
    uni, msgs, s, v, states = parity
    for kind in R.TRANSITIONS:
        assert s.transitions[kind] >= 1, kind
    w = s.lookup(uni)[2]
    assert int(np.count_nonzero(R.bits(w) == NEG_ZERO)) >= 1   # thresholded: -0.0
    assert 0 < s.entries <= uni.size
    assert sum(s.transitions.values()) == sum(m[0].size for m in msgs)


def one(alpha=1.0, beta=1.0, lambda1=1.0, lambda2=0.1, pushes=()):
    """Both restatements over pushes of one key; returns the scalar entry."""
    s, v = R.ScalarFTRL(alpha, beta, lambda1, lambda2), R.VectorFTRL(alpha, beta, lambda1, lambda2)
    for p, n, g in pushes:
        for m in (s, v):
            m.push(np.array([42], np.uint64), np.array([p], np.uint32), np.array([n], np.uint32),
                   np.array([g], np.float64))
    a, b = s.lookup([42]), v.lookup([42])
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    assert s.nnz == v.nnz
    return int(a[0][0]), int(a[1][0]), float(a[2][0]), float(a[3][0]), s.nnz


def test_first_touch_with_no_counts():
    # all == 0: both norms 0, sigma 0, lambda2 = 0.1 + (1 + 0) / 1
    pos, neg, w, z, nnz = one(pushes=[(0, 0, 3.0)])
    assert (pos, neg) == (0, 0) and z == 3.0
    assert w == -((3.0 - 1.0) / (0.1 + 1.0)) and nnz == 1


def test_threshold_gives_negative_zero():
    for g in (0.5, -0.5, 1.0, -1.0, 0.0):   # |z| <= lambda1, the bounds included
        pos, neg, w, z, nnz = one(pushes=[(1, 2, g)])
        assert fbits(w) == NEG_ZERO and z == g and nnz == 0


def test_both_signs_past_the_threshold():
    sq = math.sqrt(2.0 * 3.0 / 5.0)
    l2 = 0.1 + (1.0 + sq) / 1.0
    pos, neg, w, z, nnz = one(pushes=[(2, 3, 4.0)])
    assert w == -((4.0 - 1.0) / l2) and w < 0 and nnz == 1
    pos, neg, w, z, nnz = one(pushes=[(2, 3, -4.0)])
    assert w == -((-4.0 + 1.0) / l2) and w > 0 and nnz == 1
    # a second push with the counts unchanged (sigma = 0): the weight returns to zero
    pos, neg, w, z, nnz = one(pushes=[(2, 3, 4.0), (0, 0, -4.0 + 0.25)])
    assert (pos, neg) == (2, 3) and z == 0.25 and fbits(w) == NEG_ZERO and nnz == 0


def test_nan_and_infinite_gradients():
    pos, neg, w, z, nnz = one(pushes=[(1, 1, float("nan"))])
    assert math.isnan(z) and fbits(w) == NEG_ZERO and nnz == 0   # both comparisons fail
    pos, neg, w, z, nnz = one(pushes=[(1, 1, float("inf"))])
    assert z == math.inf and w == -math.inf and nnz == 1
    pos, neg, w, z, nnz = one(pushes=[(1, 1, float("-inf"))])
    assert z == -math.inf and w == math.inf and nnz == 1


def test_counts_pass_2_to_the_32():
    pos, neg, w, z, nnz = one(pushes=[(0xFFFFFFFF, 1, 0.5)] * 3)
    assert pos == 3 * 0xFFFFFFFF and pos > 1 << 32 and neg == 3


def test_library_exports_the_ftrl_abi():
    L = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in FTRL_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        assert C.cast(getattr(raw, name), C.c_void_p).value, name
    # argument validation needs no device
    assert L.psg_ftrl_init(None, None, 0) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_status(None, None, None, None, None) == _lib.PSG_ERR_ARG


def test_python_mirror_imports():
    from parameter_server_amd import ftrl
    for name in ("setLearningRate", "setPenalty", "setValue", "getValue", "objv", "nnz",
                 "writeToFile"):
        assert callable(getattr(ftrl.FTRLModel, name)), name
    assert ftrl.format_weight(-0.25) == "-0.25"
    assert ftrl.format_weight(1234567.0) == "1.23457e+06"   # 6 significant digits, like %g
