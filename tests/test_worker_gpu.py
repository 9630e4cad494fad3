"""GPU: the device worker step (psg_mb_*, FTRLWorker) against the
restatement in tests/worker_ref.py.

Everything is read back through psg_mb_read and compared bit for bit, except
the logit stage, whose exp and log are the device's: there the bounds are
derived (each side's exp / log within 1 ulp, 1 + e and 1 / s correctly
rounded: 2 + 1 + 1 ulp), not measured.  The largest distances seen on an
MI355X are recorded in DESIGN.md section 7."""
import ctypes as C
import functools

import numpy as np
import pytest

import ftrl_ref
import oracle_py as O
import worker_ref as R
from parameter_server_amd import _lib
from parameter_server_amd.ftrl import FTRLModel
from parameter_server_amd.worker import FTRLWorker, Minibatch, sort_tile

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    if a.dtype == np.float64:
        return b.dtype == np.float64 and a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def dev(a):
    """A host array as a device tensor (its bytes, whatever the dtype)."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    if t.numel() == 0:
        t = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def host(t, dtype, n):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()[:n * np.dtype(dtype).itemsize].view(dtype).copy()


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


def localize(mb, dic):
    d = dev(dic)
    mb.localize(d.data_ptr(), dic.size)
    mb.read("pos")  # waits: d may go
    return d


def gradient(mb, w):
    t = dev(w)
    return mb.gradient(t.data_ptr())


# ---------------------------------------------------------------- sort --
TILE = None


def tile():
    global TILE
    if TILE is None:
        TILE = sort_tile()
    return TILE


SORT_NAMES = sorted(R.sort_cases(4096))


@pytest.mark.parametrize("name", SORT_NAMES)
def test_sort_and_run_length(mb, name):
    index = R.sort_cases(tile())[name]
    rng = np.random.default_rng(index.size)
    rows = min(index.size, 37)
    offset = R.csr_of(rng, index, rows)
    mb.load(offset, index, None, np.ones(rows))
    n = mb.uniq()
    skey, spos, uniq, cnt = R.vector_count_uniq(index)
    assert n == uniq.size
    got_key, got_pos = mb.read("sorted_key"), mb.read("sorted_pos")
    assert same(got_key, skey)
    inside = got_key[1:] == got_key[:-1]
    assert np.all(got_pos[1:][inside] > got_pos[:-1][inside])  # stable
    assert same(got_pos, spos)
    assert same(mb.read("uniq_key"), uniq)
    assert same(mb.read("key_cnt"), cnt)
    start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    assert same(mb.read("run_start"), start)
    off = offset.astype(np.int64)
    row_of = np.repeat(np.arange(rows), np.diff(off)).astype(np.uint32)
    assert same(mb.read("row_of"), row_of)


def test_sort_tile_is_what_the_cases_assume():
    assert tile() >= 256 and {c.size for c in R.sort_cases(tile()).values()} >= \
        {tile() - 1, tile(), tile() + 1, 3 * tile() + 7}


# ------------------------------------------------------------ localise --
@functools.lru_cache(maxsize=None)
def zipf(binary=False, odd=False):
    return R.zipf_case(binary=binary, kinds=R.ODD_LABELS if odd else (1.0, -1.0))


DICTS = ("all", "every_other", "with_absent", "empty", "single")


@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("dname", DICTS)
def test_localize_and_count_keys(mb, dname, binary):
    offset, index, value, y = zipf(binary, odd=True)
    dic = R.dict_cases(np.unique(index))[dname]
    want = R.Step("vector", offset, index, value, y, dic)
    mb.load(offset, index, value, y)
    mb.uniq()
    localize(mb, dic)
    assert same(mb.read("remapped"), want.remapped)
    assert same(mb.read("new_offset"), want.new_offset)
    assert same(mb.read("new_index"), want.new_index)
    assert same(mb.read("new_value"), want.new_value)
    assert same(mb.read("pos"), want.pos)
    assert same(mb.read("neg"), want.neg)
    if dic.size:
        absent = ~np.isin(dic, index)
        assert not mb.read("pos")[absent].any() and not mb.read("neg")[absent].any()


# ---------------------------------------------------- ordered products --
def products(mb, case, dic, seed):
    import torch
    offset, index, value, y = case
    rng = np.random.default_rng(seed)
    x, c = R.special_vector(rng, dic.size), R.special_vector(rng, y.size)
    want = R.Step("vector", offset, index, value, y, dic)
    mb.load(offset, index, value, y)
    mb.uniq()
    d = localize(mb, dic)
    tx, tc = dev(x), dev(c)
    txw = torch.full((max(y.size, 1),), 7.0, dtype=torch.float64, device="cuda:0")
    tg = torch.full((max(dic.size, 1),), 7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    mb.times(tx.data_ptr(), txw.data_ptr())
    mb.trans_times(tc.data_ptr(), tg.data_ptr())
    mb.read("pos")  # waits
    xw = R.vector_times(want.new_offset, want.new_index, want.nv, x)
    g = R.vector_trans_times(want.new_offset, want.new_index, want.nv, c, dic.size)
    del d
    return host(txw, np.float64, y.size), xw, host(tg, np.float64, dic.size), g


@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("dname", ("all", "every_other", "with_absent"))
def test_times_and_trans_times_bit_exact(mb, dname, binary):
    case = zipf(binary)
    dic = R.dict_cases(np.unique(case[1]))[dname]
    xw, xw_ref, g, g_ref = products(mb, case, dic, 41)
    assert same(xw, xw_ref)
    assert same(g, g_ref)


def test_one_run_of_2000(mb):
    case = R.column_case()
    dic = np.unique(case[1])
    xw, xw_ref, g, g_ref = products(mb, case, dic, 43)
    assert same(xw, xw_ref)
    assert same(g, g_ref)


# --------------------------------------------------------------- logit --
def test_logit_gradient_and_objv(mb):
    offset, index, value, y = zipf()
    dic = R.dict_cases(np.unique(index))["with_absent"]
    rng = np.random.default_rng(47)
    w = rng.standard_normal(dic.size) * 2.0 ** -17
    want = R.Step("vector", offset, index, value, y, dic, w)
    assert np.abs(want.xw).max() < 30 and np.abs(want.xw).max() > 1
    mb.load(offset, index, value, y)
    mb.uniq()
    localize(mb, dic)
    objv = gradient(mb, w)
    assert same(mb.read("xw"), want.xw)  # both sides start from the same input
    tau, loss, grad = mb.read("tau"), mb.read("loss"), mb.read("grad")
    d_tau = R.ulp_distance(tau, want.tau)
    d_loss = np.abs(loss - want.loss) / (2.0 ** -52 * np.maximum(1.0, want.loss))
    gb = R.grad_bound(want, y)
    d_grad = np.abs(grad - want.grad)
    print("largest distances: tau %d ulp, loss %.3f x 2^-52 max(1, loss), grad %.3f of its bound,"
          " objv %.3g of its bound" % (d_tau.max(), d_loss.max(),
                                       np.max(d_grad[gb > 0] / gb[gb > 0]),
                                       abs(objv - want.objv) / R.objv_bound(want.loss)))
    assert d_tau.max() <= 4
    assert np.all(np.abs(loss - want.loss) <= R.loss_bound(want.loss))
    assert np.all(d_grad <= gb)
    assert abs(objv - want.objv) <= R.objv_bound(want.loss)
    again = gradient(mb, w)
    assert bits(np.float64(again)) == bits(np.float64(objv))
    assert same(mb.read("grad"), grad)


def test_empty_dictionary_and_empty_rows(mb):
    """ndict == 0: Z is empty, Xw all +0.0, loss = log 2, tau = 1/2."""
    offset, index, value, y = zipf()
    mb.load(offset, index, value, y)
    mb.uniq()
    localize(mb, np.zeros(0, np.uint64))
    objv = gradient(mb, np.zeros(0))
    assert not bits(mb.read("xw")).any()
    assert np.all(mb.read("tau") == 0.5)
    assert np.all(np.abs(mb.read("loss") - np.log(2.0)) <= 4 * 2.0 ** -52)
    assert mb.read("grad").size == 0 and mb.read("new_index").size == 0
    assert abs(objv - y.size * np.log(2.0)) <= y.size * 2.0 ** -50


# -------------------------------------------------------------- errors --
def test_errors(ctx, mb):
    L = _lib.lib()
    one = np.zeros(1, np.uint64)
    off = np.array([0, 1 << 32], np.uint64)  # sizes only
    assert L.psg_mb_load(mb._h, off.ctypes.data, 1, one.ctypes.data, None,
                         np.ones(1).ctypes.data) == _lib.PSG_ERR_SIZE
    h32 = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F32, 0, C.byref(h32)))
    assert L.psg_mb_create(h32, C.byref(C.c_void_p())) == _lib.PSG_ERR_ARG
    L.psg_destroy(h32)
    fresh = Minibatch(ctx)
    n, p = C.c_size_t(), C.c_void_p()
    assert L.psg_mb_uniq(fresh._h, None, None, C.byref(n)) == _lib.PSG_ERR_ARG
    assert L.psg_mb_localize(fresh._h, None, 0, None, None, None) == _lib.PSG_ERR_ARG
    offset, index, value, y = zipf()
    fresh.load(offset, index, value, y)
    assert L.psg_mb_localize(fresh._h, None, 0, None, None, None) == _lib.PSG_ERR_ARG
    assert L.psg_mb_gradient(fresh._h, 0, None, C.byref(p), None, None) == _lib.PSG_ERR_ARG
    fresh.uniq()
    assert L.psg_mb_gradient(fresh._h, 0, None, C.byref(p), None, None) == _lib.PSG_ERR_ARG
    assert L.psg_mb_times(fresh._h, None, None, None) == _lib.PSG_ERR_ARG
    assert L.psg_mb_read(fresh._h, _lib.PSG_MB_POS, None, 0, C.byref(n)) == _lib.PSG_ERR_ARG
    uniq = np.unique(index)
    d = localize(fresh, uniq)
    w = dev(np.zeros(uniq.size))
    assert L.psg_mb_gradient(fresh._h, 1, w.data_ptr(), C.byref(p), None, None) == \
        _lib.PSG_ERR_ARG  # an unknown loss
    assert L.psg_mb_read(fresh._h, _lib.PSG_MB_GRAD, None, 0, C.byref(n)) == _lib.PSG_ERR_ARG
    assert L.psg_mb_read(fresh._h, 99, None, 0, C.byref(n)) == _lib.PSG_ERR_ARG
    assert L.psg_mb_read(fresh._h, _lib.PSG_MB_POS, None, 0, C.byref(n)) == _lib.PSG_ERR_SIZE
    assert n.value == uniq.size
    del d
    fresh.close()


def test_unsorted_dictionary_is_reported_and_the_next_minibatch_works(mb):
    offset, index, value, y = zipf()
    uniq = np.unique(index)
    bad = uniq.copy()
    bad[[10, 11]] = bad[[11, 10]]
    mb.load(offset, index, value, y)
    mb.uniq()
    d = dev(bad)
    mb.localize(d.data_ptr(), bad.size)
    w = dev(np.zeros(bad.size))
    with pytest.raises(_lib.PSGError) as e:
        mb.gradient(w.data_ptr())
    assert e.value.status == _lib.PSG_ERR_UNSORTED
    with pytest.raises(_lib.PSGError) as e:  # localize must be called again
        mb.gradient(w.data_ptr())
    assert e.value.status == _lib.PSG_ERR_ARG
    mb.localize(d.data_ptr(), bad.size)
    with pytest.raises(_lib.PSGError) as e:  # ... and psg_mb_read reports it too
        mb.read("pos")
    assert e.value.status == _lib.PSG_ERR_UNSORTED
    want = R.Step("vector", offset, index, value, y, uniq)
    mb.load(offset, index, value, y)
    mb.uniq()
    localize(mb, uniq)
    gradient(mb, np.zeros(uniq.size))
    assert same(mb.read("pos"), want.pos) and same(mb.read("new_index"), want.new_index)


# --------------------------------------------------------------- reuse --
def test_large_small_large_on_one_handle(ctx):
    m = Minibatch(ctx)
    large = R.column_case(seed=6, rows=1500)
    small = R.zipf_case(seed=11, rows=20, mean=3)
    for offset, index, value, y in (large, small, large):
        dic = np.unique(index)[::2]
        rng = np.random.default_rng(3)
        w = rng.standard_normal(dic.size) * 2.0 ** -22
        want = R.Step("vector", offset, index, value, y, dic, w)
        m.load(offset, index, value, y)
        assert m.uniq() == want.uniq.size
        localize(m, dic)
        gradient(m, w)
        for name, ref in (("sorted_key", want.skey), ("sorted_pos", want.spos),
                          ("uniq_key", want.uniq), ("key_cnt", want.cnt),
                          ("new_offset", want.new_offset), ("new_index", want.new_index),
                          ("new_value", want.new_value), ("pos", want.pos), ("neg", want.neg),
                          ("xw", want.xw)):
            assert same(m.read(name), ref), name
        assert np.all(np.abs(m.read("grad") - want.grad) <= R.grad_bound(want, y))
    m.close()


# --------------------------------------------------------- closed loop --
CM_N, CM_K = 1 << 16, 2
PARAM = dict(alpha=0.1, beta=1.0, lambda1=0.01, lambda2=0.1)


@pytest.mark.parametrize("freq", (0, 2))
def test_closed_loop(freq):
    batches = R.closed_loop_batches()
    model = FTRLModel(0, capacity_hint=4096)
    model.setLearningRate(PARAM["alpha"], PARAM["beta"])
    model.setPenalty(PARAM["lambda1"], PARAM["lambda2"])
    worker = FTRLWorker(model, tail_feature_freq=freq, countmin_n=CM_N, countmin_k=CM_K)
    ref = ftrl_ref.ScalarFTRL(**PARAM)
    table, n, k = O.cm_resize(CM_N, CM_K)
    seen, total, num_ex = [], 0.0, 0
    for b, (offset, index, value, y) in enumerate(batches):
        objv, rows = worker.step(offset, index, value, y)
        skey, spos, uniq, cnt = R.vector_count_uniq(index)
        if freq:
            O.cm_insert(table, n, k, uniq, cnt)
            dic = O.ff_query(table, n, k, uniq, freq)
            if b == 0:  # the filter both drops and keeps
                assert 0 < dic.size < uniq.size
        else:
            dic = uniq
        assert same(worker.last_dict(), dic)
        w = worker.last_w()
        assert same(w, ftrl_ref.pull(ref, dic))  # what the model held before this push
        want = R.Step("vector", offset, index, value, y, dic, w)  # the same pulled w
        assert np.isfinite(want.loss).all()
        pos, neg, grad = worker.mb.read("pos"), worker.mb.read("neg"), worker.mb.read("grad")
        assert same(pos, want.pos) and same(neg, want.neg)
        assert np.all(np.abs(grad - want.grad) <= R.grad_bound(want, y))
        assert abs(objv - want.objv) <= R.objv_bound(want.loss)
        assert rows == y.size
        ref.push(dic, pos, neg, grad)  # the device's own message
        seen.append(dic)
        total += objv
        num_ex += rows
    assert worker.num_ex == num_ex and bits(np.float64(worker.objv)) == bits(np.float64(total))
    keys = np.unique(np.concatenate(seen))
    got, exp = model.lookup(keys), ref.lookup(keys)
    for g, e in zip(got, exp):
        assert same(np.asarray(g), np.asarray(e))
    assert got[4].all()
    worker.close()
    model.close()
