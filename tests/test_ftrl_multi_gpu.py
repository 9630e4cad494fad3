"""GPU: m FTRL models in one pass (psg_ftrlm_*, psg_mb_*_rows, FTRLMultiModel,
FTRLMultiWorker).  Every column is held bit for bit to the scalar path or to
the restatements of tests/worker_ref.py and tests/ftrl_ref.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import ftrl_ref
import worker_ref as R
from parameter_server_amd import _lib
from parameter_server_amd.ftrl import FTRLModel, FTRLMultiModel
from parameter_server_amd.worker import FTRLMultiWorker, FTRLWorker, Minibatch

pytestmark = pytest.mark.gpu

MS = (1, 3, 8, 32)  # G = 1, idle lanes in the group, a full group, two keys per wave
U64MAX = (1 << 64) - 1


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def host(t, shape):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.float64)[:int(np.prod(shape))].reshape(shape).copy()


@pytest.fixture(scope="module")
def ctx():
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    yield h
    L.psg_destroy(h)


@pytest.fixture(scope="module")
def mb(ctx):
    m = Minibatch(ctx)
    yield m
    m.close()


CASES = {"zipf": lambda: R.zipf_case(binary=False), "zipf_binary": lambda: R.zipf_case(binary=True),
         "column": R.column_case}


@functools.lru_cache(maxsize=None)
def localized(cname, dname):
    """(case, dictionary, its Step): Z does not depend on the model."""
    case = CASES[cname]()
    dic = R.dict_cases(np.unique(case[1]))[dname]
    return case, dic, R.Step("vector", *case, dic)


def load(mb, case, dic):
    mb.load(*case)
    mb.uniq()
    d = dev(dic)
    mb.localize(d.data_ptr(), dic.size)
    mb.read("pos")  # waits: d may go


def columns(rng, n, m, gen=R.special_vector):
    return np.ascontiguousarray(np.stack([gen(rng, n) for _ in range(m)], axis=1))


# 1 ------------------------------------------------------------ row products --
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("dname", ("all", "every_other"))
@pytest.mark.parametrize("cname", sorted(CASES))
def test_row_products_bit_exact_per_column(mb, cname, dname, m):
    import torch
    case, dic, want = localized(cname, dname)
    rows = case[3].size
    nv = None if case[2] is None else want.new_value
    rng = np.random.default_rng(100 + m)
    x, c = columns(rng, dic.size, m), columns(rng, rows, m)
    assert m == 1 or not np.array_equal(bits(x[:, 0]), bits(x[:, 1]))
    load(mb, case, dic)
    tx, tc = dev(x), dev(c)
    txw = torch.full((rows * m,), 7.0, dtype=torch.float64, device="cuda:0")
    tg = torch.full((dic.size * m,), 7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    mb.times_rows(tx.data_ptr(), m, txw.data_ptr())
    mb.trans_times_rows(tc.data_ptr(), m, tg.data_ptr())
    mb.read("pos")  # waits
    xw, g = host(txw, (rows, m)), host(tg, (dic.size, m))
    for j in range(m):
        xw_ref = R.vector_times(want.new_offset, want.new_index, nv, x[:, j])
        g_ref = R.vector_trans_times(want.new_offset, want.new_index, nv, c[:, j], dic.size)
        assert np.array_equal(bits(xw[:, j]), bits(xw_ref)), "Xw column %d" % j
        assert np.array_equal(bits(g[:, j]), bits(g_ref)), "gradient column %d" % j


# 2 ----------------------------------------------------------- gradient_rows --
@pytest.mark.parametrize("m", MS)
def test_gradient_rows_is_m_scalar_gradients(mb, m):
    case, dic, _ = localized("zipf", "every_other")
    w = np.random.default_rng(200 + m).standard_normal((dic.size, m)) * 2.0 ** -17
    load(mb, case, dic)
    scalar = []
    for j in range(m):
        t = dev(w[:, j])
        objv = mb.gradient(t.data_ptr())
        scalar.append((objv, mb.read("tau"), mb.read("grad")))
    t = dev(w)
    objv = mb.gradient_rows(t.data_ptr(), m)
    tau, grad = mb.read_rows("tau"), mb.read_rows("grad")
    assert tau.shape == (case[3].size, m) and grad.shape == (dic.size, m)
    for j, (o, ta, gr) in enumerate(scalar):
        assert bits(np.float64(objv[j])) == bits(np.float64(o)), "objv of column %d" % j
        assert np.array_equal(bits(tau[:, j]), bits(ta)), "tau column %d" % j
        assert np.array_equal(bits(grad[:, j]), bits(gr)), "gradient column %d" % j


# 3 ------------------------------------------------------------------ server --
def sweep(m):
    """m settings that differ; column m // 2 has a lambda1 large enough that
    many of its weights threshold to -0.0 (grad = 2 N(0,1))."""
    p = [dict(alpha=0.5 + 0.1 * j, beta=1.0 + 0.05 * j, lambda1=0.1 * j, lambda2=0.1 + 0.01 * j)
         for j in range(m)]
    p[m // 2]["lambda1"] = 4.0
    return p


def messages(m, seed=1, universe=400):
    """(universe, messages of sizes 1, 64/G - 1, 64/G + 1, 257 and two of 100):
    keys overlap, keys 0 and 2^64 - 1 are in the 257 and in a later message."""
    rng = np.random.default_rng(seed)
    uni = np.unique(np.concatenate([rng.integers(1, 1 << 63, size=universe, dtype=np.uint64),
                                    np.array([0, U64MAX], np.uint64)]))
    per_wave = 64 >> int(math.ceil(math.log2(m)))
    msgs = []
    for n, ends in ((1, False), (max(per_wave - 1, 1), False), (per_wave + 1, False), (257, True),
                    (100, True), (100, False)):
        k = rng.choice(uni[1:-1], size=n - 2 * ends, replace=False)
        k = np.sort(np.concatenate([k, uni[[0, -1]]]) if ends else k)
        msgs.append((k, rng.integers(0, 6, size=n).astype(np.uint32),
                     rng.integers(0, 6, size=n).astype(np.uint32),
                     2.0 * rng.standard_normal((n, m))))
    return uni, msgs


@pytest.mark.parametrize("m", MS)
def test_server_columns_match_scalar_models(m):
    params = sweep(m)
    uni, msgs = messages(m)
    # 4 keys of room: the messages of 64/G + 1 (or 257) and 257 keys each pass
    # the limit, so the index is rebuilt at least twice
    model = FTRLMultiModel(params, capacity_hint=4)
    refs = [ftrl_ref.ScalarFTRL(**p) for p in params]
    for k, pos, neg, grad in msgs:
        model.push(k, pos, neg, grad)
        for j, ref in enumerate(refs):
            ref.push(k, pos, neg, grad[:, j])
    probe = np.concatenate([uni, ftrl_ref.absent_keys(uni, 20)])
    pos, neg, w, z, found = model.lookup(probe)
    entries, nnz, norm1, norm2 = model.status()
    assert entries == refs[0].entries
    for j, ref in enumerate(refs):
        rp, rn, rw, rz, rf = ref.lookup(probe)
        assert np.array_equal(pos, rp) and np.array_equal(neg, rn) and np.array_equal(found, rf)
        assert np.array_equal(bits(w[:, j]), bits(rw)), "w column %d" % j
        assert np.array_equal(bits(z[:, j]), bits(rz)), "z column %d" % j
        assert nnz[j] == ref.nnz
        s1, s2 = math.fsum(np.abs(rw)), math.fsum(rw * rw)
        assert abs(norm1[j] - s1) <= entries * 2.0 ** -53 * s1
        assert abs(norm2[j] - s2) <= entries * 2.0 ** -53 * s2  # rw * rw rounds as the device's
        ek, ew = model.export(j)
        keep = rw[:uni.size] != 0
        assert np.array_equal(ek, uni[keep]) and np.array_equal(bits(ew), bits(rw[:uni.size][keep]))
    thresholded = w[found == 1, m // 2]
    assert np.any((thresholded == 0) & np.signbit(thresholded))
    mixed = np.concatenate([probe[::3], probe[:50], probe[:5]])  # absent and repeated keys
    got = model.pull(mixed)
    for j, ref in enumerate(refs):
        assert np.array_equal(bits(got[:, j]), bits(ftrl_ref.pull(ref, mixed)))
    model.close()


# 4 ---------------------------------------------------------------- unsorted --
def test_unsorted_message_applies_nothing_and_is_reported_once():
    m = 3
    params = sweep(m)
    uni, msgs = messages(m, seed=2)
    model = FTRLMultiModel(params, capacity_hint=1024)
    refs = [ftrl_ref.ScalarFTRL(**p) for p in params]
    k, pos, neg, grad = msgs[3]
    bad = k.copy()
    bad[[10, 11]] = bad[[11, 10]]
    model.push(bad, pos, neg, grad)
    assert not model.lookup(uni)[4].any()  # lookup neither reports nor clears
    with pytest.raises(_lib.PSGError) as e:
        model.status()
    assert e.value.status == _lib.PSG_ERR_UNSORTED
    assert model.status()[0] == 0  # reported once
    model.push(k, pos, neg, grad)
    for j, ref in enumerate(refs):
        ref.push(k, pos, neg, grad[:, j])
        assert np.array_equal(bits(model.lookup(uni)[2][:, j]), bits(ref.lookup(uni)[2]))
    assert model.status()[0] == k.size
    model.close()


# 5 ------------------------------------------------------------- closed loop --
@pytest.mark.parametrize("freq", (0, 2))
def test_closed_loop_against_three_scalar_workers(freq):
    m = 3
    params = sweep(m)
    cm = dict(tail_feature_freq=freq, countmin_n=1 << 12, countmin_k=2)
    multi = FTRLMultiModel(params, capacity_hint=64)
    worker = FTRLMultiWorker(multi, **cm)
    scalar = []
    for p in params:
        model = FTRLModel(0, capacity_hint=64)
        model.setLearningRate(p["alpha"], p["beta"])
        model.setPenalty(p["lambda1"], p["lambda2"])
        scalar.append((model, FTRLWorker(model, **cm)))
    seen = []
    for offset, index, value, y in R.closed_loop_batches():
        objv, rows = worker.step(offset, index, value, y)
        assert rows == y.size and objv.shape == (m,)
        for j, (_, wk) in enumerate(scalar):
            o, _ = wk.step(offset, index, value, y)
            assert bits(np.float64(objv[j])) == bits(np.float64(o)), "objv of column %d" % j
        assert np.array_equal(worker.last_dict(), scalar[0][1].last_dict())
        seen.append(np.unique(index))
    keys = np.unique(np.concatenate(seen))
    pos, neg, w, z, found = multi.lookup(keys)
    assert 0 < found.sum() and (freq or found.all())
    for j, (model, wk) in enumerate(scalar):
        sp, sn, sw, sz, sf = model.lookup(keys)
        assert np.array_equal(pos, sp) and np.array_equal(neg, sn) and np.array_equal(found, sf)
        assert np.array_equal(bits(w[:, j]), bits(sw)) and np.array_equal(bits(z[:, j]), bits(sz))
        assert bits(np.float64(worker.objv[j])) == bits(np.float64(wk.objv))
        wk.close()
        model.close()
    worker.close()
    multi.close()


# 6 --------------------------------------------------------------- arguments --
def test_arguments(ctx):
    L = _lib.lib()
    p = (_lib.FtrlParam * 33)(*[_lib.FtrlParam(1.0, 1.0, 0.0, 0.0)] * 33)
    one, n = np.zeros(1, np.uint64), C.c_size_t()
    out = np.zeros(33, np.float64)
    fresh = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(fresh)))
    for call in (lambda: L.psg_ftrlm_reserve(fresh, 10),
                 lambda: L.psg_ftrlm_pull(fresh, one.ctypes.data, 1, out.ctypes.data),
                 lambda: L.psg_ftrlm_status(fresh, C.byref(n), None, None, None),
                 lambda: L.psg_ftrlm_export(fresh, 0, None, None, 0, C.byref(n))):
        assert call() == _lib.PSG_ERR_ARG  # before psg_ftrlm_init
    assert L.psg_ftrlm_init(fresh, p, 0, 0) == _lib.PSG_ERR_ARG
    assert L.psg_ftrlm_init(fresh, p, 33, 0) == _lib.PSG_ERR_ARG
    assert L.psg_ftrlm_init(fresh, p, 32, 16) == _lib.PSG_OK
    assert L.psg_ftrlm_export(fresh, 32, None, None, 0, C.byref(n)) == _lib.PSG_ERR_ARG
    L.psg_destroy(fresh)
    h32 = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F32, 0, C.byref(h32)))
    assert L.psg_ftrlm_init(h32, p, 2, 0) == _lib.PSG_ERR_ARG
    L.psg_destroy(h32)
    m = Minibatch(ctx)
    m.load(*R.zipf_case())
    m.uniq()
    g = C.c_void_p()
    assert L.psg_mb_times_rows(m._h, None, 2, None, None) == _lib.PSG_ERR_ARG  # before localize
    assert L.psg_mb_trans_times_rows(m._h, None, 2, None, None) == _lib.PSG_ERR_ARG
    assert L.psg_mb_gradient_rows(m._h, 0, None, 2, C.byref(g), None, None) == _lib.PSG_ERR_ARG
    dic = np.unique(R.zipf_case()[1])
    load(m, R.zipf_case(), dic)
    w = dev(np.zeros((dic.size, 33)))
    for bad in (0, 33):
        assert L.psg_mb_gradient_rows(m._h, 0, w.data_ptr(), bad, C.byref(g), None, None) == \
            _lib.PSG_ERR_ARG
    assert L.psg_mb_rows_read(m._h, _lib.PSG_MB_ROWS_TAU, None, 0, C.byref(n)) == _lib.PSG_ERR_ARG
    assert L.psg_mb_gradient_rows(m._h, 1, w.data_ptr(), 2, C.byref(g), None, None) == \
        _lib.PSG_ERR_ARG  # an unknown loss
    m.close()
