"""GPU: the device-array forms of the server context (psg_push_dev,
psg_pull_dev, psg_darling_update_dev, psg_darling_progress, psg_dev_status)
and the pass driver built on them (darling.darling_pass).

Every comparison is against the host form (psg_push, psg_gather,
psg_darling_update, DarlingWorker.gradients / update_dual) on a twin context
fed the same data, and equality is bit for bit on the raw bytes, NaN payloads
and -0.0 included: both sides run the same fold, update and worker kernels on
the same inputs in the same order, so no tolerance applies.  The one derived
bound is psg_darling_progress's objv (include/psg.h): n * 2^-53 * sum |w|.

Server keys: 2,500 seeded keys per channel -- positions [1000, 2200) are
consecutive integers, so that psg_push's own dense test accepts the slice the
claim test pushes.  2,500 slots cross the 1,024-slot tile bound twice and the
2,048-slot sparse tile bound once."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from parameter_server_amd import DarlingWorker, _lib
from parameter_server_amd.darling import darling_pass, pass_schedule, server_progress
from parameter_server_amd.kv_vector import KEY_ALL, KVVector, Message

pytestmark = pytest.mark.gpu

NKEYS = 2500
RUN = (1000, 2200)  # positions of the consecutive run
ONES = np.array([0xFFFFFFFFFFFFFFFF], np.uint64).view(np.float64)[0]
NAN2 = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
KMAX = (1 << 64) - 1


def distinct(rng, lo, hi, n):
    """n distinct sorted keys of [lo, hi)."""
    u = np.unique(rng.integers(lo, hi, size=2 * n, dtype=np.uint64))
    return np.sort(rng.choice(u, size=n, replace=False))


def server_keys(seed=11):
    rng = np.random.default_rng(seed)
    a = distinct(rng, 1, 1 << 40, RUN[0])
    b = np.uint64(1 << 41) + np.arange(RUN[1] - RUN[0], dtype=np.uint64)
    c = distinct(rng, 1 << 42, 1 << 62, NKEYS - RUN[1])
    k = np.concatenate([a, b, c])
    assert k.size == NKEYS and np.all(k[1:] > k[:-1])
    return k


K = server_keys()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """A host array in device memory, `off` bytes past a 16-byte bound."""

    def __init__(self, a, off=0):
        a = np.ascontiguousarray(a)
        self.dtype, self.n, self.off = a.dtype, a.size, off
        self.t = torch.zeros(a.nbytes + 32, dtype=torch.uint8, device="cuda:0")
        assert self.t.data_ptr() % 16 == 0
        if a.nbytes:
            self.t[off:off + a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()))
        self.ptr = self.t.data_ptr() + off

    def host(self):
        b = self.t[self.off:self.off + self.n * self.dtype.itemsize].cpu().numpy()
        return b.view(self.dtype).copy()


def dkeys(k, off=0):
    return Dev(np.ascontiguousarray(k, np.uint64), off)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.view(np.uint8), b.view(np.uint8))


def status_of(fn):
    try:
        fn()
    except _lib.PSGError as e:
        return e.status
    return _lib.PSG_OK


def values(rng, n, dtype, special=True):
    """Random values with -0.0, NaNs with payloads and an infinity among them."""
    v = (rng.standard_normal(n) * 3).astype(dtype)
    if special and n >= 7:
        u = v.view(np.uint32 if dtype == np.float32 else np.uint64)
        at = rng.permutation(n)[:4]
        v[at[0]] = -0.0
        v[at[1]] = np.inf
        if dtype == np.float32:
            u[at[2]], u[at[3]] = 0x7FC00123, 0xFFFFFFFF
        else:
            u[at[2]], u[at[3]] = 0x7FF8000000000123, 0xFFFFFFFFFFFFFFFF
    elif special:
        v[0] = -0.0
    return v


def pair(dtype, parallel=False):
    """A context and its twin, both holding K on channel 0."""
    out = []
    for _ in range(2):
        v = KVVector(0, dtype, parallel_match=parallel)
        v.setValue(Message(key=K))
        out.append(v)
    return out


def push_dev(v, t, keys, vals, key_range=KEY_ALL, slice=None, koff=0, voff=0):
    """psg_push_dev of host arrays staged in device memory; returns the
    staging buffers (the caller keeps or overwrites them)."""
    dk = dkeys(keys, koff)
    dv = [Dev(x, voff) for x in vals]
    v.push_dev(0, t, key_range, dk.ptr, dk.n, [x.ptr for x in dv], slice=slice, stream=stream())
    return [dk] + dv


def received(v, t):
    return [a for _, a in v.received(t)]


# ---------------------------------------------------------- 1. push parity --
@pytest.mark.parametrize("parallel", (False, True))
@pytest.mark.parametrize("dtype", (_lib.PSG_F32, _lib.PSG_F64))
def test_push_parity(dtype, parallel):
    """Three pushes of growing m, the second through psg_push, folded across a
    launch seam: the aggregate equals the all-psg_push twin's."""
    npd = np.float32 if dtype == _lib.PSG_F32 else np.float64
    rng = np.random.default_rng(100 + dtype)
    v, twin = pair(dtype, parallel)
    try:
        for x in (v, twin):
            x.set_flush_pushes(2)
        keep = []
        for p, (n, m) in enumerate(((1, 1), (7, 3), (1500, 1))):
            keys = np.sort(rng.choice(K, size=n, replace=False))
            vals = [values(rng, n, npd) for _ in range(m)]
            twin.setValue(Message(time=4, key=keys, value=vals))
            if p == 1:  # a host push into the same aggregate
                v.setValue(Message(time=4, key=keys, value=vals))
            else:
                keep.append(push_dev(v, 4, keys, vals))
        got, want = received(v, 4), received(twin, 4)
        assert len(got) == len(want) == 3
        for g, w in zip(got, want):
            assert g.size == NKEYS and same(g, w)
        assert np.isnan(want[0]).any() and np.count_nonzero(want[2]) >= 5  # 7 less -0.0
    finally:
        v.close()
        twin.close()


# --------------------------------------------------- 2. alignment and reuse --
@pytest.mark.parametrize("n", (1, 3, 129))
@pytest.mark.parametrize("dtype", (_lib.PSG_F32, _lib.PSG_F64))
def test_alignment_and_reuse(dtype, n):
    """Arrays one element past a 16-byte bound, overwritten with NaN on the
    caller's stream right after the call: the context took its copy."""
    npd = np.float32 if dtype == _lib.PSG_F32 else np.float64
    rng = np.random.default_rng(200 + n)
    v, twin = pair(dtype)
    try:
        keys = np.sort(rng.choice(K, size=n, replace=False))
        vals = [values(rng, n, npd) for _ in range(2)]
        twin.setValue(Message(time=1, key=keys, value=vals))
        bufs = push_dev(v, 1, keys, vals, koff=8, voff=npd().itemsize)
        assert all(b.ptr % 16 == b.off != 0 for b in bufs)
        for b in bufs:
            b.t.fill_(255)  # all-ones: NaN in both types, on the same stream
        got, want = received(v, 1), received(twin, 1)
        assert len(got) == 2 and all(same(g, w) for g, w in zip(got, want))
    finally:
        v.close()
        twin.close()


# ------------------------------------------------------------ 3. slice claim --
def test_slice_claim():
    rng = np.random.default_rng(300)
    v, twin = pair(_lib.PSG_F64)
    try:
        a, n = 1000, 1200
        keys = K[a:a + n]
        vals = [values(rng, n, np.float64), values(rng, n, np.float64)]
        extra = np.sort(rng.choice(K, size=40, replace=False))  # a sparse push beside it
        ev = [values(rng, 40, np.float64), values(rng, 40, np.float64)]
        # a true claim; the twin's psg_push finds the same slice by its dense test
        for t, second in ((1, False), (2, True)):
            twin.setValue(Message(time=t, key=keys, value=vals))
            keep = push_dev(v, t, keys, vals, slice=a)
            if second:  # dense and sparse pushes in one aggregate
                twin.setValue(Message(time=t, key=extra, value=ev))
                keep += push_dev(v, t, extra, ev)
            got, want = received(v, t), received(twin, t)
            assert all(same(g, w) for g, w in zip(got, want))
        # one differing key: reported like an unmatched key
        wrong = keys.copy()
        wrong[777] += np.uint64(1 << 50)
        keep = push_dev(v, 3, wrong, vals, slice=a)
        assert status_of(lambda: v.received(3)) == _lib.PSG_ERR_UNMATCHED
        # the right keys at the wrong place
        keep = push_dev(v, 4, keys, vals, slice=a + 1)
        assert status_of(lambda: v.received(4)) == _lib.PSG_ERR_UNMATCHED
        # a claim past hi, or before lo: at the call
        assert status_of(lambda: push_dev(v, 5, keys, vals, slice=NKEYS - n + 1)) == \
            _lib.PSG_ERR_ARG
        assert status_of(lambda: push_dev(v, 5, keys[:10], [x[:10] for x in vals],
                                          key_range=(int(K[1005]), KMAX), slice=1000)) == \
            _lib.PSG_ERR_ARG
        assert status_of(lambda: v.received(5)) == _lib.PSG_ERR_NO_TIME
        # unsorted device keys without a claim, as for psg_push
        uns = np.sort(rng.choice(K, size=50, replace=False))
        uns[[10, 30]] = uns[[30, 10]]
        uv = [values(rng, 50, np.float64)]
        twin.setValue(Message(time=6, key=uns, value=uv))
        keep = push_dev(v, 6, uns, uv)
        assert status_of(lambda: twin.received(6)) == _lib.PSG_ERR_UNMATCHED
        assert status_of(lambda: v.received(6)) == _lib.PSG_ERR_UNMATCHED
        assert status_of(v.dev_status) == _lib.PSG_OK
    finally:
        v.close()
        twin.close()


# ------------------------------------------------------------ 4. pull parity --
@pytest.mark.parametrize("dtype", (_lib.PSG_F32, _lib.PSG_F64))
def test_pull_parity(dtype):
    npd = np.float32 if dtype == _lib.PSG_F32 else np.float64
    rng = np.random.default_rng(400)
    v, twin = pair(dtype)
    try:
        w = values(rng, NKEYS, npd)
        for x in (v, twin):
            x.set_value_array(0, w)
        for n in (1, 3000):
            present = rng.choice(K, size=n - n // 3, replace=True)  # repeats
            absent = rng.integers(1, 1 << 63, size=n // 3, dtype=np.uint64)
            req = np.sort(np.concatenate([present, absent]))
            msg = Message(key=req)
            matched = twin.getValue(msg)
            dk = dkeys(req, 8)
            out = Dev(np.full(n, 7, npd), npd().itemsize)
            cnt = Dev(np.array([12345], np.uint64))
            v.pull_dev(0, dk.ptr, n, out.ptr, cnt.ptr, stream=stream())
            torch.cuda.synchronize()
            assert same(out.host(), msg.value[0])
            assert int(cnt.host()[0]) == matched
            if n > 1:
                assert 0 < matched < n
        assert status_of(v.dev_status) == _lib.PSG_OK
        # an unsorted request: reported once
        req = np.sort(rng.choice(K, size=1500, replace=False))
        req[[100, 1400]] = req[[1400, 100]]
        dk, out = dkeys(req), Dev(np.zeros(req.size, npd))
        v.pull_dev(0, dk.ptr, req.size, out.ptr, None, stream=stream())
        assert status_of(lambda: twin.getValue(Message(key=req))) == _lib.PSG_ERR_UNSORTED
        assert status_of(v.dev_status) == _lib.PSG_ERR_UNSORTED
        assert status_of(v.dev_status) == _lib.PSG_OK
    finally:
        v.close()
        twin.close()


# ----------------------------------------------- 5. update and progress --
PARAM = {"eta": 0.7, "lambda_": 0.5, "kkt_filter_threshold": 0.2}
DELTA_MAX = 5.0
BLOCKS5 = ((0, 9), (1000, 1060), (2030, NKEYS))  # server positions


def darling_state(v, n=NKEYS):
    delta, active = np.empty(n), np.empty(n, np.uint8)
    nnz = C.c_size_t()
    _lib.check(v._L.psg_darling_state(v._h, 0, 0, n, delta.ctypes.data, active.ctypes.data,
                                      C.byref(nnz)))
    return delta, active, nnz.value


def host_update(v, t):
    p = _lib.DarlingParam(PARAM["eta"], PARAM["lambda_"], PARAM["kkt_filter_threshold"],
                          DELTA_MAX)
    vio = C.c_double()
    _lib.check(v._L.psg_darling_update(v._h, 0, t, C.cast(C.byref(p), C.c_void_p), C.byref(vio)))
    return vio.value


def dev_update(v, t):
    p = _lib.DarlingParam(PARAM["eta"], PARAM["lambda_"], PARAM["kkt_filter_threshold"],
                          DELTA_MAX)
    _lib.check(v._L.psg_darling_update_dev(v._h, 0, t, C.cast(C.byref(p), C.c_void_p)))


def key_range_of(a, b):
    return int(K[a]), int(K[b]) if b < NKEYS else KMAX


def test_update_and_progress():
    rng = np.random.default_rng(500)
    v, twin = pair(_lib.PSG_F64)
    try:
        w0 = np.where(rng.random(NKEYS) < 0.5, 0.0, rng.standard_normal(NKEYS))
        for x in (v, twin):
            x.set_value_array(0, w0)
            _lib.check(x._L.psg_darling_init(x._h, 0, 1.0))
        vios, keep = [], []
        other = torch.cuda.Stream()
        for i, (a, b) in enumerate(BLOCKS5):
            G = rng.standard_normal(b - a)
            U = rng.uniform(0.05, 2.0, b - a)
            kr = key_range_of(a, b)
            twin.setValue(Message(time=3 * i, key_range=kr, key=K[a:b], value=[G, U]))
            vios.append(host_update(twin, 3 * i))
            keep.append(push_dev(v, 3 * i, K[a:b], [G, U], key_range=kr,
                                 slice=a if i == 1 else None))
            dev_update(v, 3 * i)
            # the ordering rule: a pull called after the update, on another
            # stream, sees the updated values
            dk, out = dkeys(K[a:b]), Dev(np.zeros(b - a))
            other.wait_stream(torch.cuda.current_stream())  # the request was staged there
            v.pull_dev(0, dk.ptr, b - a, out.ptr, None, stream=other.cuda_stream)
            other.synchronize()
            msg = Message(key=K[a:b])
            twin.getValue(msg)
            assert same(out.host(), msg.value[0])
            assert not same(msg.value[0], w0[a:b])
        assert max(vios) > 0 and len(set(vios)) == 3
        pr = server_progress(v, 0, PARAM["lambda_"])
        assert same(np.array([pr["violation"]]), np.array([max(vios)]))
        assert same(v.value(0), twin.value(0))
        (d1, a1, n1), (d2, a2, n2) = darling_state(v), darling_state(twin)
        assert same(d1, d2) and same(a1, a2) and n1 == n2 == pr["nnz_active"] < NKEYS
        # reset_violation reads, then zeroes
        assert server_progress(v, 0, 0.5, reset_violation=True)["violation"] == max(vios)
        assert server_progress(v, 0, 0.5)["violation"] == 0.0

        # progress over every kind of weight
        w = rng.standard_normal(NKEYS) * np.exp2(rng.integers(-30, 30, NKEYS))
        at = rng.permutation(NKEYS)
        w[at[:40]] = ONES
        w[at[40:50]] = NAN2
        w[at[50:90]] = 0.0
        w[at[90:120]] = -0.0
        w[at[120:140]] = 5e-324 * rng.integers(1, 1 << 40, 20)
        w[at[140:150]] = -5e-324
        v.set_value_array(0, w)
        live = ~np.isnan(w) & (w != 0)
        lam = 0.5
        pr = server_progress(v, 0, lam)
        assert pr["nnz_w"] == int(live.sum()) == NKEYS - 120
        assert pr["nnz_active"] == n2
        exact = math.fsum(np.abs(w[live]).tolist())
        bound = NKEYS * 2.0 ** -53 * exact
        err = abs(pr["objv"] - lam * exact)
        print("progress objv: %.3g of its bound" % (err / bound))
        assert err <= bound
        again = server_progress(v, 0, lam)
        assert same(np.array([again["objv"]]), np.array([pr["objv"]])) and again == pr

        # a block with an unmatched push: the model is untouched
        a, b = 300, 340
        bad = K[a:b - 1].copy()
        bad[5] += np.uint64(1)
        assert bad[5] not in K
        before = (v.value(0), *darling_state(v))
        keep.append(push_dev(v, 30, bad, [np.ones(b - a - 1), np.ones(b - a - 1)],
                             key_range=key_range_of(a, b)))
        dev_update(v, 30)
        assert status_of(lambda: v.received(30)) == _lib.PSG_ERR_NO_TIME  # erased
        assert status_of(v.dev_status) == _lib.PSG_ERR_UNMATCHED
        assert status_of(v.dev_status) == _lib.PSG_OK
        after = (v.value(0), *darling_state(v))
        assert all(same(np.asarray(x), np.asarray(y)) for x, y in zip(before, after))
    finally:
        v.close()
        twin.close()


# ------------------------------------------------------------ 6. pass parity --
def worker_data(rng, dic, binary, rows=150, per_row=30):
    idx = [np.sort(rng.choice(dic, size=per_row, replace=False)) for _ in range(rows)]
    offset = np.arange(rows + 1, dtype=np.uint64) * np.uint64(per_row)
    index = np.concatenate(idx)
    value = None if binary else \
        rng.choice([-1.0, 1.0], index.size) * (0.5 + rng.random(index.size))
    return offset, index, value, rng.choice([-1.0, 1.0], rows)


def pass_case(binary, seed=600):
    """Two workers' dictionaries over 2,300 server keys (the union), their
    rows, and the key blocks of the pass."""
    rng = np.random.default_rng(seed)
    S = distinct(rng, 1, 1 << 62, 2300)
    in0 = rng.random(S.size) < 0.6
    in1 = ~in0 | (rng.random(S.size) < 0.2)
    in0[1500:1520], in1[1500:1520] = True, False  # only worker 0 holds these
    dicts = [S[in0], S[in1]]
    data = [worker_data(rng, d, binary) for d in dicts]
    blocks = [(int(S[0]), int(S[9])),           # 9 keys
              (int(S[1000]), int(S[1060])),     # straddles position 1,024
              (int(S[2030]), int(S[2080])),     # straddles position 2,048
              (int(S[1500]), int(S[1520])),     # one worker only
              (int(S[1600]) + 1, int(S[1601])), # no key at all
              (int(S[1060]), int(S[1500])),
              (int(S[2080]), KMAX)]
    return S, dicts, data, blocks


def host_pass(server, workers, t, blocks, param):
    """The schedule of darling_pass through setValue, psg_darling_update,
    getValue and update_dual."""
    p = _lib.DarlingParam(param["eta"], param["lambda_"], param["kkt_filter_threshold"],
                          DELTA_MAX)
    vio = 0.0
    for (kb, ke), row in zip(blocks, pass_schedule([w.dict_keys for w in workers], blocks)):
        if not row:
            continue
        for i, cb, ce in row:
            G, U = workers[i].gradients(cb, ce)
            server.setValue(Message(time=t, key_range=(kb, ke), key=workers[i].dict_keys[cb:ce],
                                    value=[G, U]))
        x = C.c_double()
        _lib.check(server._L.psg_darling_update(server._h, 0, t, C.cast(C.byref(p), C.c_void_p),
                                                C.byref(x)))
        vio = max(vio, x.value)
        for i, cb, ce in row:
            msg = Message(key=workers[i].dict_keys[cb:ce])
            server.getValue(msg)
            workers[i].update_dual(cb, ce, msg.value[0])
        t += 3
    return t, vio


@pytest.mark.parametrize("binary", (False, True))
def test_pass_parity(binary):
    S, dicts, data, blocks = pass_case(binary)
    assert S.size >= 2049 and np.intersect1d(dicts[0], dicts[1]).size >= 1
    assert np.array_equal(np.union1d(dicts[0], dicts[1]), S)
    sched = pass_schedule(dicts, blocks)
    assert [len(r) for r in sched][:5] == [2, 2, 2, 1, 0]
    servers, workers = [], []
    try:
        for _ in range(2):
            v = KVVector(0, _lib.PSG_F64)
            servers.append(v)
            v.setValue(Message(key=S))
            v.set_value_array(0, np.zeros(S.size))
            _lib.check(v._L.psg_darling_init(v._h, 0, 1.0))
            ws = []
            for d, (offset, index, value, y) in zip(dicts, data):
                w = DarlingWorker(v._h, 1.0, DELTA_MAX)
                workers.append(w)
                w.load(offset, index, value, y, d)
                ws.append(w)
            v.workers = ws
        dev, host = servers
        first = {"eta": 1.0, "lambda_": 1.0, "kkt_filter_threshold": 1e20}
        second = dict(first, kkt_filter_threshold=0.1)
        t_dev = t_host = 0
        for n, param in enumerate((first, second)):
            t_dev = darling_pass(dev, dev.workers, 0, t_dev, blocks, param)
            t_host, vio = host_pass(host, host.workers, t_host, blocks, param)
            assert t_dev == t_host == 3 * 6 * (n + 1)
            pr = server_progress(dev, 0, param["lambda_"], reset_violation=True)
            assert same(np.array([pr["violation"]]), np.array([vio]))
            assert same(dev.value(0), host.value(0))
            sd, sh = darling_state(dev, S.size), darling_state(host, S.size)
            assert same(sd[0], sh[0]) and same(sd[1], sh[1]) and sd[2] == sh[2] == pr["nnz_active"]
            for wd, wh in zip(dev.workers, host.workers):
                a, b = wd.state(), wh.state()
                for name in ("dual", "cur_w", "delta", "active", "delta_w"):
                    assert same(a[name], b[name]), name
            if n == 0:
                assert sd[2] == S.size and np.count_nonzero(dev.value(0)) > 0
        # the second pass deactivated some columns and left others active
        assert 0 < sd[2] < S.size
        assert any(0 < int(w.state()["active"].sum()) < w.ndict for w in dev.workers)
    finally:
        for w in workers:
            w.close()
        for v in servers:
            v.close()

