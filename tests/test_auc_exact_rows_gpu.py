"""GPU: the exact rank AUC of a sweep (psg_auc_exact_rows*, exact_auc_rows,
FTRLMultiWorker.exact_auc) against a plain NumPy restatement of
Evaluation<double>::auc and against the scalar exact_auc, column by column.

Every comparison is of the float64's bits (NaN against NaN): the area is an
integer and the two divisions and the flip are the scalar path's, so there is
no tolerance to derive."""
import ctypes as C
import math

import numpy as np
import pytest

import worker_ref as W
from parameter_server_amd import _lib
from parameter_server_amd.auc import exact_auc, exact_auc_rows
from parameter_server_amd.ftrl import FTRLMultiModel
from parameter_server_amd.worker import FTRLMultiWorker, sort_tile

pytestmark = pytest.mark.gpu

F64 = np.float64
SHAPES = ("1x1", "T-1x3", "Tx2", "T+1x5", "Sx4", "S+1x32", "2S+3x7")
INPUTS = ("distinct", "ties_and_zeros", "constant_high_bytes", "all_positive")


def shape_of(name):
    t, s = int(_lib.lib().psg_auc_exact_rows_tile()), sort_tile()
    return {"1x1": (1, 1), "T-1x3": (t - 1, 3), "Tx2": (t, 2), "T+1x5": (t + 1, 5), "Sx4": (s, 4),
            "S+1x32": (s + 1, 32), "2S+3x7": (2 * s + 3, 7)}[name]


def reference(y, p):
    """evaluation.h:17-44 of one column: a stable sort, the positives before
    each negative as integers, two float64 divisions and the flip."""
    order = np.argsort(p + 0.0, kind="stable")  # -0.0 + 0.0 is +0.0
    pos = y[order] > 0
    before = np.cumsum(pos, dtype=np.uint64) - pos.astype(np.uint64)
    area, npos = int(before[~pos].sum(dtype=np.uint64)), int(pos.sum())
    with np.errstate(invalid="ignore"):
        a = F64(area) / (F64(npos) * F64(y.size - npos))
    return 1 - a if a < 0.5 else a


def bits(v):
    return "nan" if math.isnan(v) else int(F64(v).view(np.uint64))


@pytest.fixture(scope="module")
def ctx():
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    yield h
    L.psg_destroy(h)


@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_column_is_the_scalar_exact_auc(ctx, shape, inputs):
    n, m = shape_of(shape)
    rng = np.random.default_rng(SHAPES.index(shape) * 10 + INPUTS.index(inputs))
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0)
    if inputs == "ties_and_zeros":
        p = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25]), size=(n, m))
    else:
        p = rng.normal(0, 3, (n, m)) + 0.5 * y[:, None]
    if inputs == "constant_high_bytes":  # beside columns of both signs (if m > 1)
        p[:, 0] = 1.0 + rng.random(n)
    if inputs == "all_positive":
        y[:] = 1.0
    got = exact_auc_rows(ctx, y, p)
    assert got.shape == (m,)
    for j in range(m):
        col = np.ascontiguousarray(p[:, j])
        assert bits(got[j]) == bits(reference(y, col)) == bits(exact_auc(ctx, y, col)), "model %d" % j
        assert math.isnan(got[j]) == bool((y > 0).all() or (y <= 0).all())  # one class absent


@pytest.mark.parametrize("column", (0, 3, 4))
def test_a_nan_names_its_column(ctx, column):
    n, m = sort_tile() + 1, 5
    rng = np.random.default_rng(column)
    y, p = np.where(rng.random(n) < 0.5, 1.0, -1.0), rng.normal(0, 1, (n, m))
    p[[7, n - 1], column] = np.nan
    out = np.full(m, -7.0)
    L = _lib.lib()
    assert L.psg_auc_exact_rows(ctx, y.ctypes.data, p.ctypes.data, n, m,
                                out.ctypes.data) == _lib.PSG_ERR_ARG
    msg = L.psg_last_error().decode()
    assert "column %d has 2 NaN" % column in msg and (out == -7.0).all()  # auc unwritten


def test_errors(ctx):
    L = _lib.lib()
    y, p, out = np.ones(4), np.ones(4 * 33), np.zeros(33)
    for bad in (0, _lib.PSG_FTRL_MAX_MODELS + 1):
        assert L.psg_auc_exact_rows(ctx, y.ctypes.data, p.ctypes.data, 4, bad,
                                    out.ctypes.data) == _lib.PSG_ERR_ARG
    assert L.psg_auc_exact_rows(ctx, y.ctypes.data, p.ctypes.data, (1 << 32) // 2, 2,
                                out.ctypes.data) == _lib.PSG_ERR_SIZE
    with pytest.raises(ValueError):
        exact_auc_rows(ctx, y, np.ones(4))  # 1-D
    assert np.isnan(exact_auc_rows(ctx, np.zeros(0), np.zeros((0, 3)))).all()  # 0 / 0


def test_multi_worker_exact_auc_scores_and_leaves_the_model():
    params = [dict(alpha=0.5 + 0.1 * j, beta=1.0, lambda1=0.1 * j, lambda2=0.1) for j in range(3)]
    batches = W.closed_loop_batches()[:3]
    model = FTRLMultiModel(params, capacity_hint=64)
    worker = FTRLMultiWorker(model)
    for b in batches[:2]:
        worker.step(*b)
    before = model.status()
    got = worker.exact_auc(*batches[2])
    after = model.status()
    assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1:], after[1:]))
    want = exact_auc_rows(model._model(), batches[2][3], worker.predict(*batches[2]))
    assert [bits(v) for v in got] == [bits(v) for v in want] and not np.isnan(got).any()
    worker.close()
    model.close()
