"""GPU: device-resident evaluation (psg_auc_*, psg_auc_exact*, psg_mb_labels,
FTRLWorker.predict and step(auc=)) against the restatement in
tests/auc_ref.py.

Everything is compared exactly: the histogram's keys and counts as integers,
every double by its bits (all NaNs one value: 0 / 0 carries no payload worth
keeping).  No step here has a rounding that the device could make
differently from the host -- the key is one rounded multiply and a
truncation, every count is an integer, accuracy and evaluate are the
library's host code -- so there is no tolerance to derive."""
import ctypes as C
import math

import numpy as np
import pytest

import auc_ref as R
import worker_ref as W
from parameter_server_amd import _lib
from parameter_server_amd.auc import AUC, accuracy_data, evaluate_data, exact_auc, exact_auc_dev
from parameter_server_amd.ftrl import FTRLModel
from parameter_server_amd.worker import FTRLWorker, sort_tile

pytestmark = pytest.mark.gpu

I64, U64, F64 = np.int64, np.uint64, np.float64
NAMES = sorted(R.add_cases(2048))        # the names do not depend on the tile
EXACT_NAMES = sorted(R.exact_cases(2048))
PARAM = dict(alpha=0.1, beta=1.0, lambda1=0.01, lambda2=0.1)
_CASES = {}


def cases(kind):
    """The cases at the library's own sort tile, computed once."""
    if kind not in _CASES:
        _CASES[kind] = (R.add_cases if kind == "add" else R.exact_cases)(sort_tile())
    return _CASES[kind]


def fbits(v):
    return "nan" if math.isnan(v) else int(R.bits(F64(v))[0])


def dev(a):
    """A host array as a device tensor (its bytes, whatever the dtype)."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    if t.numel() == 0:
        t = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def ctx():
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    yield h
    L.psg_destroy(h)


@pytest.fixture(scope="module")
def auc(ctx):
    """One handle for the whole module: every test also tests clear and reuse."""
    a = AUC(ctx, 1000)
    yield a
    a.close()


def fresh(auc, goodness):
    auc.clear()
    auc.setGoodness(goodness)
    return auc


def add_dev(auc, y, p):
    ty, tp = dev(y), dev(p)
    auc.add_dev(ty.data_ptr(), tp.data_ptr(), y.size)
    return auc.data()  # waits: the tensors may go


# ------------------------------------------------------------------- add --
def test_sizes_sit_around_the_sort_tile():
    t = sort_tile()
    assert [n for _, n in R.sizes(t)] == [1, t - 1, t, t + 1, 3 * t + 5]
    y, p, g = cases("add")["seam_run"]
    k = np.sort(R.vector_keys(p, g))
    run = np.nonzero(k == k[t])[0]
    assert run[0] < t <= run[-1]  # one key's run straddles the first seam
    assert len(set(R.bits(y[np.argsort(R.vector_keys(p, g), kind="stable")][run]).tolist())) > 2
    assert np.unique(R.vector_keys(*cases("add")["one_key"][1:])).size == 1
    d = cases("add")["distinct"]
    assert np.unique(R.vector_keys(d[1], d[2])).size == 3 * t + 5


@pytest.mark.parametrize("name", NAMES)
def test_add_dev_matches_compute(auc, name):
    y, p, g = cases("add")[name]
    got = add_dev(fresh(auc, g), y, p)
    assert R.same_data(got, R.vector_compute(y, p, g))


def test_special_predictions_by_hand(auc):
    p = np.array([0.4, -0.4, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, 2.0 ** 63, -2.0 ** 63,
                  2.0 ** 62, -2.5])
    y = np.array([1, -1, 1, 0.0, 1, 1, -0.0, np.nan, 2.5, 1, -1, 1])
    tk, tc, fk, fc = add_dev(fresh(auc, 1), y, p)
    assert tk.tolist() == [R.INT64_MIN, -2, 0] and tc.tolist() == [4, 1, 2]
    assert fk.tolist() == [R.INT64_MIN, 0, 1 << 62] and fc.tolist() == [2, 2, 1]


@pytest.mark.parametrize("name", ("mixed_3Tp5_g10", "distinct"))
def test_batching(auc, name):
    """One call, and five uneven pieces with an empty one: keys that overlap
    between the pieces (mixed) and disjoint key sets (distinct, sorted)."""
    y, p, g = cases("add")[name]
    if name == "distinct":
        o = np.argsort(p)
        y, p = y[o], p[o]
    t = sort_tile()
    cuts = [0, 100, 100, t + 3, 2 * t, y.size]
    pieces = [(y[a:b], p[a:b]) for a, b in zip(cuts, cuts[1:])]
    pieces = [pieces[i] for i in (3, 0, 1, 4, 2)]  # later keys first: inserts on both sides
    whole = add_dev(fresh(auc, g), y, p)
    assert R.same_data(whole, R.vector_compute(y, p, g))
    fresh(auc, g)
    keep = [(dev(a), dev(b), a.size) for a, b in pieces]
    for ta, tb, n in keep:
        auc.add_dev(ta.data_ptr(), tb.data_ptr(), n)
    assert R.same_data(auc.data(), whole)
    fresh(auc, g)  # host arrays, and the handle again after clear
    for a, b in pieces:
        auc.add(a, b)
    assert R.same_data(auc.data(), whole)


def test_grows_past_its_first_capacity(ctx):
    a = AUC(ctx, 1)
    n = 40000  # two adds of distinct keys pass the first 65536 entries
    ys, ps = [], []
    for part in range(3):
        p = np.arange(part, 3 * n, 3, dtype=F64)
        y = np.where(np.arange(n) % 3 == 0, 1.0, -1.0)
        a.add(y, p)
        ys.append(y)
        ps.append(p)
    assert R.same_data(a.data(), R.vector_compute(np.concatenate(ys), np.concatenate(ps), 1))
    a.close()


# ----------------------------------------------------------------- merge --
def test_merge(auc):
    y, p, g = cases("add")["mixed_Tp1_g10"]
    mine = R.vector_compute(y, p, g)
    big = 1 << 40
    hit_t, hit_f = int(mine[0][3]), int(mine[2][5])  # keys the add also hits
    other = (np.array([hit_t, 777777, -5, hit_t, 555555, -5, R.INT64_MIN], I64),
             np.array([big, 2, 0, 5, 0, 3, (1 << 63)], U64),
             np.array([hit_f, 12, hit_f, (1 << 63) - 1, 12], I64),
             np.array([big, 1, big, 9, 0], U64))
    want = R.vector_merge([mine, other])
    assert R.same_data(want, R.scalar_merge([mine, other]))
    at = want[0].tolist().index(hit_t)
    assert int(want[1][at]) == big + 5 + int(mine[1][3]) > 1 << 32
    assert 555555 not in want[0].tolist()  # only zero counts: no key
    fresh(auc, g)
    auc.merge(*other)
    auc.add(y, p)
    assert R.same_data(auc.data(), want)
    fresh(auc, g)
    auc.add(y, p)
    auc.merge(*other)
    auc.merge(np.zeros(0, I64), np.zeros(0, U64), np.zeros(0, I64), np.zeros(0, U64))
    assert R.same_data(auc.data(), want)


# ------------------------------------------------- accuracy and evaluate --
@pytest.mark.parametrize("name", ("mixed_3Tp5_g10", "mixed_Tp1_g100000", "one_key", "distinct"))
def test_accuracy_and_evaluate_equal_the_host_functions_on_the_export(auc, name):
    y, p, g = cases("add")[name]
    data = add_dev(fresh(auc, g), y, p)
    for th in (0.0, 0.5, -0.5):
        assert fbits(auc.accuracy(th)) == fbits(accuracy_data(g, *data, threshold=th)) \
            == fbits(R.scalar_accuracy(data, g, th))
    for as_written in (False, True):
        assert fbits(auc.evaluate(as_written)) == fbits(evaluate_data(*data, as_written=as_written)) \
            == fbits(R.scalar_evaluate(data, as_written))


def test_empty_histogram_and_errors(ctx, auc):
    L = _lib.lib()
    fresh(auc, 10)
    assert all(a.size == 0 for a in auc.data())
    assert math.isnan(auc.accuracy()) and auc.evaluate() == 0.5
    auc.add(np.zeros(0), np.zeros(0))  # n == 0: a legal no-op
    assert all(a.size == 0 for a in auc.data())
    auc.add(np.ones(3), np.array([0.1, 0.2, 0.3]))
    assert L.psg_auc_set_goodness(auc._h, 100) == _lib.PSG_ERR_ARG  # not empty
    assert auc.data()[0].tolist() == [1, 2, 3]
    nt, nf = C.c_size_t(), C.c_size_t()
    assert L.psg_auc_data(auc._h, None, None, 0, C.byref(nt), None, None, 0, C.byref(nf)) == \
        _lib.PSG_ERR_SIZE
    assert (nt.value, nf.value) == (3, 0)
    assert L.psg_auc_add_dev(auc._h, None, None, (1 << 32) - 1, None) == _lib.PSG_ERR_ARG
    one = dev(np.ones(1))
    assert L.psg_auc_add_dev(auc._h, one.data_ptr(), one.data_ptr(), (1 << 32) - 1, None) == \
        _lib.PSG_ERR_SIZE
    v = C.c_double()
    assert L.psg_auc_evaluate(auc._h, 5, C.byref(v)) == _lib.PSG_ERR_ARG
    assert L.psg_auc_create(ctx, 10, None) == _lib.PSG_ERR_ARG


# ------------------------------------------------------------- exact AUC --
@pytest.mark.parametrize("name", EXACT_NAMES)
def test_exact_auc(ctx, name):
    y, p = cases("exact")[name]
    want = R.vector_exact(y, p)
    got = exact_auc(ctx, y, p)
    assert fbits(got) == fbits(want)
    if name.startswith("all_"):
        assert math.isnan(got)
    if name.startswith("distinct") and not math.isnan(want):
        # all predictions distinct: the reference's own formula over any sort
        o = np.argsort(p)
        pos = y[o] > 0
        area = float((np.cumsum(pos) - pos)[~pos].sum()) / (float(pos.sum()) * float((~pos).sum()))
        assert fbits(got) == fbits(1 - area if area < 0.5 else area)


def test_exact_auc_zeros_are_one_value(ctx):
    for y, p in (([1.0, -1.0], [-0.0, 0.0]), ([1.0, -1.0], [0.0, -0.0]),
                 ([-1.0, 1.0], [-0.0, 0.0]), ([-1.0, 1.0], [0.0, -0.0])):
        assert exact_auc(ctx, np.array(y), np.array(p)) == 1.0 == R.scalar_exact(y, p)
    # two examples give 1.0 either way round (0 flips to 1).  Three do not:
    # in input order the negative has one positive before it, 1 / 2; a key
    # that put -0.0 below +0.0 would put both positives first, 2 / 2
    y, p = np.array([1.0, -1.0, 1.0]), np.array([-0.0, 0.0, -0.0])
    assert exact_auc(ctx, y, p) == R.scalar_exact(y, p) == 0.5


def test_exact_auc_dev_nan_and_sizes(ctx):
    y, p = cases("exact")["ties_seam"]
    ty, tp = dev(y), dev(p)
    assert fbits(exact_auc_dev(ctx, ty.data_ptr(), tp.data_ptr(), y.size)) == \
        fbits(R.vector_exact(y, p))
    bad = p.copy()
    bad[sort_tile() + 1] = np.nan
    with pytest.raises(_lib.PSGError) as e:
        exact_auc(ctx, y, bad)
    assert e.value.status == _lib.PSG_ERR_ARG
    assert math.isnan(exact_auc(ctx, np.zeros(0), np.zeros(0)))
    v = C.c_double()
    assert _lib.lib().psg_auc_exact_dev(ctx, ty.data_ptr(), tp.data_ptr(), (1 << 32) - 1,
                                        C.byref(v), None) == _lib.PSG_ERR_SIZE


# ------------------------------------------ predict and step(..., auc=) --
def new_model():
    model = FTRLModel(0, capacity_hint=4096)
    model.setLearningRate(PARAM["alpha"], PARAM["beta"])
    model.setPenalty(PARAM["lambda1"], PARAM["lambda2"])
    return model, FTRLWorker(model)


def trained(nsteps):
    """A model that the first `nsteps` closed-loop batches have trained."""
    batches = W.closed_loop_batches()
    model, worker = new_model()
    for offset, index, value, y in batches[:nsteps]:
        worker.step(offset, index, value, y)
    return batches, model, worker


def test_predict_scores_without_touching_the_model():
    batches, model, worker = trained(3)
    before = (model.status(), model.export())
    assert before[0][0] > 0 and before[0][1] > 0
    for offset, index, value, y in (batches[3], batches[0]):  # unseen keys, and seen ones
        xw_dev = worker.predict(offset, index, value, y)
        y_dev, xw_own = worker.mb.labels()
        assert xw_dev == xw_own and xw_dev
        dic = np.unique(index)
        assert np.array_equal(worker.last_dict(), dic)
        w = worker.last_w()
        assert np.array_equal(R.bits(w), R.bits(model_pull(model, dic)))
        want = W.Step("vector", offset, index, value, y, dic, w).xw
        got = worker.mb.read("xw")
        assert got.shape == want.shape and np.array_equal(R.bits(got), R.bits(want))
        assert np.any(got != 0)
    after = (model.status(), model.export())
    assert before[0][:2] == after[0][:2]
    assert np.array_equal(R.bits(np.array(before[0][2:])), R.bits(np.array(after[0][2:])))
    assert np.array_equal(before[1][0], after[1][0])
    assert np.array_equal(R.bits(before[1][1]), R.bits(after[1][1]))
    worker.close()
    model.close()


def model_pull(model, keys):
    from parameter_server_amd.kv_vector import Message
    msg = Message(key=keys)
    model.getValue(msg)
    return msg.value[-1]


def test_step_with_auc_is_progressive_validation_and_leaves_the_model_alone():
    g = 100000
    batches, plain, pw = trained(len(W.closed_loop_batches()))  # the run without the keyword
    model, worker = new_model()
    a = AUC(model._model(), g)
    seen = []
    for offset, index, value, y in batches:
        worker.step(offset, index, value, y, auc=a)
        seen.append((y.copy(), worker.mb.read("xw")))
    want = R.vector_compute(np.concatenate([s[0] for s in seen]),
                            np.concatenate([s[1] for s in seen]), g)
    assert R.same_data(a.data(), want)
    assert R.same_data(want, R.vector_merge([R.vector_compute(y, xw, g) for y, xw in seen]))
    assert want[0].size > 1 and want[2].size > 1
    keys = np.unique(np.concatenate([b[1] for b in batches]))
    for x, z in zip(model.lookup(keys), plain.lookup(keys)):
        x, z = np.asarray(x), np.asarray(z)
        assert x.dtype == z.dtype and np.array_equal(x.view(np.uint8), z.view(np.uint8))
    assert model.status()[:2] == plain.status()[:2]
    assert worker.num_ex == pw.num_ex and fbits(worker.objv) == fbits(pw.objv)
    a.close()
    worker.close()
    pw.close()
    model.close()
    plain.close()
