"""GPU: the row-valued AUC (psg_auc_rows_*, AUCRows, FTRLMultiWorker.step's
auc=) against the restatement in tests/auc_ref.py, column by column.

As in test_auc_gpu.py every comparison is exact: keys and counts as integers,
doubles by their bits; model j must be what a scalar histogram fed column j
alone holds, so there is no tolerance to derive."""
import ctypes as C
import math

import numpy as np
import pytest

import auc_ref as R
import worker_ref as W
from parameter_server_amd import _lib
from parameter_server_amd.auc import AUC, AUCRows
from parameter_server_amd.ftrl import FTRLModel, FTRLMultiModel
from parameter_server_amd.worker import FTRLMultiWorker, FTRLWorker, sort_tile

pytestmark = pytest.mark.gpu

F64 = np.float64
SIZES = ("m", "Tm1", "T", "Tp1", "3Tp5")  # n * m, around the sort tile T
ADD_CASES = [(m, s) for m in (1, 2, 3, 32) for s in SIZES] + [(3, "nTp1")]


def rows_of(m, size):
    t = sort_tile()
    if size == "nTp1":  # n itself past a tile: a row and a run straddle the seam
        return t + 1
    target = {"m": m, "Tm1": t - 1, "T": t, "Tp1": t + 1, "3Tp5": 3 * t + 5}[size]
    return -(-target // m)


def fbits(v):
    return "nan" if math.isnan(v) else int(R.bits(F64(v))[0])


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, F64).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def batch(seed, n, m):
    """(y[n], predict[n, m]): every column from its own generator."""
    p = np.stack([np.random.default_rng(1000 * seed + j).normal(0, 3, n) for j in range(m)], axis=1)
    return R.mixed_labels(np.random.default_rng(seed), n), p


@pytest.fixture(scope="module")
def ctx():
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    yield h
    L.psg_destroy(h)


def add_all(a, batches):
    """The first batch through add_dev, the others through the host add."""
    for i, (y, p) in enumerate(batches):
        if i == 0:
            ty, tp = dev(y), dev(p)
            a.add_dev(ty.data_ptr(), tp.data_ptr(), y.size)
            a.data(0)  # waits: the tensors may go
        else:
            a.add(y, p)


def expected(batches, g, j):
    return R.vector_compute(np.concatenate([y for y, _ in batches]),
                            np.concatenate([p[:, j] for _, p in batches]), g)


def assert_columns(a, batches, g):
    for j in range(a.m):
        assert R.same_data(a.data(j), expected(batches, g, j)), "model %d" % j


# 1 --------------------------------------------------------------------- add --
@pytest.mark.parametrize("g", (10, 100000))
@pytest.mark.parametrize("m,size", ADD_CASES)
def test_two_adds_match_compute_per_column(ctx, m, size, g):
    n = rows_of(m, size)
    batches = [batch(1, n, m), batch(2, n, m)]  # the second meets resident entries
    a = AUCRows(ctx, m, g)
    add_all(a, batches[:1])
    assert_columns(a, batches[:1], g)
    add_all(a, batches)  # the first again (every key resident), then the second
    assert_columns(a, [batches[0]] + batches, g)
    a.close()


# 2 ---------------------------------------------------------------- segments --
def test_segments_grow_unevenly(ctx):
    n = sort_tile() + 1
    rng = np.random.default_rng(7)
    i = np.arange(n, dtype=F64)
    same = np.round(rng.normal(0, 300, n))
    first = np.stack([np.full(n, 0.5), rng.permutation(i), -1.0 - rng.permutation(i), same], axis=1)
    second = np.stack([np.full(n, 0.5), rng.permutation(i) + n // 2, 10.0 * n + rng.permutation(i),
                       same], axis=1)
    batches = [(R.mixed_labels(rng, n), first), (R.mixed_labels(rng, n), second)]
    assert first[:, 2].max() < first[:, 1].min() and second[:, 2].min() > second[:, 1].max()
    a = AUCRows(ctx, 4, 1)
    add_all(a, batches)
    assert_columns(a, batches, 1)
    want = [expected(batches, 1, j) for j in range(4)]
    assert np.union1d(want[0][0], want[0][2]).size == 1  # one key
    assert np.union1d(want[1][0], want[1][2]).size == n + n // 2
    a.close()


# 3 --------------------------------------------------------------- wide span --
def test_wide_span_goes_model_by_model_and_narrow_adds_follow(ctx):
    m, n = 32, 2 * sort_tile()
    y, p = batch(3, n, m)
    p[[5, n // 2], 4] = [np.nan, 1e300]  # both key to INT64_MIN
    p[:, 9] = np.random.default_rng(9).uniform(-9.2e18, 9.2e18, n)
    keys = R.vector_keys(p, 1)
    assert int(keys.max()) - int(keys.min()) >= 1 << 63  # b = 64: no room for 5 model bits
    batches = [(y, p), batch(4, n, m)]
    a = AUCRows(ctx, m, 1)
    add_all(a, batches[:1])
    assert_columns(a, batches[:1], 1)
    add_all(a, [batches[1]])
    assert_columns(a, batches, 1)
    a.close()


# 4 ---------------------------------------------------- merge and the doubles --
def test_merge_accuracy_and_evaluate(ctx):
    m, g, n = 3, 10, sort_tile() + 1
    mine, other = batch(5, n, m), batch(6, n, m)
    a = AUCRows(ctx, m, g)
    add_all(a, [mine])
    want = []
    for j in (2, 0, 1):
        theirs = R.vector_compute(other[0], other[1][:, j], g)
        a.merge(j, *theirs)
        want.append((j, R.vector_merge([expected([mine], g, j), theirs])))
    for j, w in want:
        assert R.same_data(a.data(j), w)
    want = [w for _, w in sorted(want, key=lambda x: x[0])]
    acc, by_key, written = a.accuracy(0.0), a.evaluate(), a.evaluate(as_written=True)
    raw = (C.c_double * m)()
    for j, w in enumerate(want):
        assert fbits(acc[j]) == fbits(R.vector_accuracy(w, g, 0.0))
        assert fbits(by_key[j]) == fbits(R.vector_evaluate(w))
        assert fbits(written[j]) == fbits(R.vector_evaluate(w, as_written=True))
    _lib.check(a._L.psg_auc_rows_accuracy(a._h, 0.0, raw))
    assert [fbits(v) for v in raw] == [fbits(v) for v in acc]
    _lib.check(a._L.psg_auc_rows_evaluate(a._h, _lib.PSG_AUC_AS_WRITTEN, raw))
    assert [fbits(v) for v in raw] == [fbits(v) for v in written]
    a.close()


# 5 ------------------------------------------------------- the scalar handle --
def test_model_j_is_a_scalar_handle_fed_column_j(ctx):
    m, g = 3, 100000
    n = rows_of(m, "3Tp5")
    batches = [batch(1, n, m), batch(2, n, m)]
    a = AUCRows(ctx, m, g)
    add_all(a, batches)
    for j in range(m):
        s = AUC(ctx, g)
        for y, p in batches:
            s.add(y, p[:, j])
        assert R.same_data(a.data(j), s.data())
        s.close()
    a.close()


# 6 ------------------------------------------------------------------ worker --
def test_multi_worker_keeps_every_models_progressive_auc():
    m, g = 3, 100000
    params = [dict(alpha=0.5 + 0.1 * j, beta=1.0 + 0.05 * j, lambda1=0.1 * j, lambda2=0.1)
              for j in range(m)]
    batches = W.closed_loop_batches()[:3]
    multi, plain = FTRLMultiModel(params, capacity_hint=64), FTRLMultiModel(params, capacity_hint=64)
    worker, bare = FTRLMultiWorker(multi), FTRLMultiWorker(plain)
    a = AUCRows(multi._model(), m, g)
    scalar = []
    for p in params:
        model = FTRLModel(0, capacity_hint=64)
        model.setLearningRate(p["alpha"], p["beta"])
        model.setPenalty(p["lambda1"], p["lambda2"])
        scalar.append((model, FTRLWorker(model), AUC(model._model(), g)))
    for offset, index, value, y in batches:
        objv, _ = worker.step(offset, index, value, y, auc=a)
        assert np.array_equal(R.bits(objv), R.bits(bare.step(offset, index, value, y)[0]))
        for _, wk, s in scalar:
            wk.step(offset, index, value, y, auc=s)
    for j, (model, wk, s) in enumerate(scalar):
        got = a.data(j)
        assert got[0].size > 1 and got[2].size > 1 and R.same_data(got, s.data())
        s.close()
        wk.close()
        model.close()
    wrong = AUCRows(multi._model(), m + 1, g)
    with pytest.raises(ValueError):
        worker.step(*batches[0], auc=wrong)
    for h in (wrong, a, worker, bare, multi, plain):
        h.close()


# 7 ------------------------------------------------------------------ errors --
def test_errors(ctx):
    L = _lib.lib()
    h = C.c_void_p()
    for bad in (0, _lib.PSG_FTRL_MAX_MODELS + 1):
        assert L.psg_auc_rows_create(ctx, 10, bad, C.byref(h)) == _lib.PSG_ERR_ARG
    a = AUCRows(ctx, 2, 10)
    a.add(np.zeros(0), np.zeros((0, 2)))  # n == 0: a legal no-op
    a.setGoodness(100)
    a.add(np.ones(3), np.array([[0.01, 0.5], [0.02, 0.5], [0.03, 0.5]]))
    assert L.psg_auc_rows_set_goodness(a._h, 10) == _lib.PSG_ERR_ARG  # not empty
    nt, nf = C.c_size_t(), C.c_size_t()
    key, cnt = np.full(2, -7, np.int64), np.full(2, 7, np.uint64)
    assert L.psg_auc_rows_data(a._h, 0, key.ctypes.data, cnt.ctypes.data, 2, C.byref(nt), None,
                               None, 0, C.byref(nf)) == _lib.PSG_ERR_SIZE
    assert (nt.value, nf.value) == (3, 0) and key.tolist() == [-7, -7]  # nothing copied
    assert a.data(1)[0].tolist() == [50] and a.data(1)[1].tolist() == [3]
    for j in (-1, 2):
        assert L.psg_auc_rows_data(a._h, j, None, None, 0, C.byref(nt), None, None, 0,
                                   C.byref(nf)) == _lib.PSG_ERR_ARG
        assert L.psg_auc_rows_merge(a._h, j, None, None, 0, None, None, 0) == _lib.PSG_ERR_ARG
    one = dev(np.ones(2))
    assert L.psg_auc_rows_add_dev(a._h, one.data_ptr(), one.data_ptr(), 1 << 31, None) == \
        _lib.PSG_ERR_SIZE  # n * m >= 2^32 - 1
    a.clear()
    assert all(x.size == 0 for j in range(2) for x in a.data(j))
    a.close()
