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
def products(mb, case, dic, seed, want=None):
    """want: the case's Step against dic where it is there already (Z does
    not depend on the values, so the valued case's serves the binary one)."""
    import torch
    offset, index, value, y = case
    rng = np.random.default_rng(seed)
    x, c = R.special_vector(rng, dic.size), R.special_vector(rng, y.size)
    if want is None:
        want = R.Step("vector", offset, index, value, y, dic)
    nv = None if value is None else want.new_value
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
    xw = R.vector_times(want.new_offset, want.new_index, nv, x)
    g = R.vector_trans_times(want.new_offset, want.new_index, nv, c, dic.size)
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
    logit_checks(mb, (offset, index, value, y), dic, w, want)


def logit_checks(mb, case, dic, w, want):
    """psg_mb_gradient of `case` against `want`, its Step with weights w."""
    offset, index, value, y = case
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
        whole_step(m, (offset, index, value, y), dic, w)
    m.close()


def whole_step(m, case, dic, w, want=None):
    """Load to gradient on handle m, every array against the restatement."""
    offset, index, value, y = case
    if want is None:
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


# ------------------------------------------------------- the seam case --
# One minibatch past the first iteration of every second-level structure of
# the kernels (worker_ref.seam_case; tests/test_worker.py asserts what it
# reaches).  Its reference step is computed once, and it has a handle of its
# own, so the shared one keeps the small buffers the other tests grew.
SEAM_SEED = 29


class Seam:
    def __init__(self, ctx):
        self.case = R.seam_case(tile(), SEAM_SEED)
        offset, index, value, y = self.case
        self.binary_case = (offset, index, None, y)
        self.dic = R.seam_dict(index)
        self.w = np.random.default_rng(47).standard_normal(self.dic.size) * 2.0 ** -19
        self.want = R.Step("vector", offset, index, value, y, self.dic, self.w)
        self.mb = Minibatch(ctx)


@pytest.fixture(scope="module")
def seam(ctx):
    s = Seam(ctx)
    yield s
    s.mb.close()


def test_seam_sort_and_run_lengths(seam):
    """More than 256 tiles, a tile count that is no multiple of 8, all eight
    digit passes: row_scan_kernel's second trip and carry in every pass and
    in the run heads' scan, xcd_index as a permutation."""
    offset, index, value, y = seam.case
    want, m = seam.want, seam.mb
    m.load(offset, index, value, y)
    assert m.uniq() == want.uniq.size
    got_key, got_pos = m.read("sorted_key"), m.read("sorted_pos")
    assert same(got_key, want.skey)
    assert same(got_pos, want.spos)
    assert same(m.read("uniq_key"), want.uniq)
    assert same(m.read("key_cnt"), want.cnt)
    start = np.concatenate([[0], np.cumsum(want.cnt)]).astype(np.uint32)
    assert same(m.read("run_start"), start)
    row_of = np.repeat(np.arange(y.size), np.diff(offset.astype(np.int64))).astype(np.uint32)
    assert same(m.read("row_of"), row_of)


def test_seam_localize_and_count_keys(seam):
    """Kept and dropped pairs on both sides of flag tile 256: the
    compaction's scan carries."""
    offset, index, value, y = seam.case
    want, m, dic = seam.want, seam.mb, seam.dic
    m.load(offset, index, value, y)
    m.uniq()
    localize(m, dic)
    assert same(m.read("remapped"), want.remapped)
    assert same(m.read("new_offset"), want.new_offset)
    assert same(m.read("new_index"), want.new_index)
    assert same(m.read("new_value"), want.new_value)
    assert same(m.read("pos"), want.pos)
    assert same(m.read("neg"), want.neg)
    absent = ~np.isin(dic, index)
    assert absent.sum() >= 50
    assert not m.read("pos")[absent].any() and not m.read("neg")[absent].any()


@pytest.mark.parametrize("binary", (False, True))
def test_seam_times_and_trans_times_bit_exact(seam, binary):
    """More long runs than the long-run kernel has waves, and a run at every
    edge of the short / long split and of a chain_sum batch."""
    case = seam.binary_case if binary else seam.case
    xw, xw_ref, g, g_ref = products(seam.mb, case, seam.dic, 59, seam.want)
    assert same(xw, xw_ref)
    assert same(g, g_ref)
    if binary:
        assert seam.mb.read("new_value").size == 0


def test_seam_logit_gradient_and_objv(seam):
    """More than 256 partial sums of the objective; the bounds' premise
    n < 2^20 holds (test_worker.py asserts it of the case)."""
    logit_checks(seam.mb, seam.case, seam.dic, seam.w, seam.want)


def test_seam_then_small_on_one_handle(seam):
    whole_step(seam.mb, seam.case, seam.dic, seam.w, seam.want)
    offset, index, value, y = R.zipf_case(seed=11, rows=20, mean=3)
    dic = np.unique(index)[::2]
    w = np.random.default_rng(3).standard_normal(dic.size) * 2.0 ** -22
    whole_step(seam.mb, (offset, index, value, y), dic, w)


@pytest.mark.parametrize("binary", (False, True))
def test_run_edges(mb, binary):
    """A run of exactly each length around kLongRun, a wave, and one and two
    batches of chain_sum; two dictionary keys with no run (+0.0)."""
    offset, index, value, y, dic = R.run_edge_case(binary=binary)
    want = R.Step("vector", offset, index, value, y, dic)
    assert sorted(want.cnt.tolist()) == sorted(R.RUN_EDGES)
    xw, xw_ref, g, g_ref = products(mb, (offset, index, value, y), dic, 61, want)
    assert same(xw, xw_ref)
    assert same(g, g_ref)
    absent = ~np.isin(dic, index)
    assert absent.sum() == 2 and not bits(g)[absent].any()
    assert same(mb.read("pos") + mb.read("neg"),
                np.where(absent, 0, np.bincount(np.searchsorted(dic, index),
                                                minlength=dic.size)).astype(np.uint32))


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
