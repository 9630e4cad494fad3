"""GPU: Darling for m settings in one pass (psg_mb_darling_rows_*,
psg_darling_rows_*, DarlingMultiWorker / DarlingMultiServer /
darling_pass_rows) against m runs of the scalar device path, which column j
must equal bit for bit, and against the host restatement
(tests/darling_worker_ref.py) under the bounds the scalar tests hold the
device to: G, cur_w, delta, delta_w and the mask bit for bit, U, dual and objv
within D.u_bound, D.dual_bound and D.objv_bound.  m = 1, 3 and 32: a group of
one lane, a group with an idle lane, a full half-wave."""
import ctypes as C

import numpy as np
import pytest

import darling_worker_ref as D
import oracle_py as O
from parameter_server_amd import (DarlingMultiServer, DarlingMultiWorker, DarlingWorker, _lib,
                                  darling_pass_rows)
from parameter_server_amd.darling import darling_pass
from parameter_server_amd.kv_vector import KVVector, Message
from parameter_server_amd.worker import Minibatch

pytestmark = pytest.mark.gpu

DELTA_INIT = 1.0
RANGES = ((0, 60), D.INNER)
ONES = 0xFFFFFFFFFFFFFFFF
MS = (1, 3, 32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return b.dtype == np.float64 and a.shape == b.shape and \
            np.array_equal(D.bits(a), D.bits(b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def within(got, want, bound):
    """Every item equal (infinities included), NaN on both sides, or inside its bound."""
    got, want, bound = np.asarray(got), np.asarray(want), np.asarray(bound)
    with np.errstate(all="ignore"):
        ok = (np.isnan(got) & np.isnan(want)) | (got == want) | (np.abs(got - want) <= bound)
    return bool(np.all(ok))


@pytest.fixture(scope="module")
def ctx():
    v = KVVector(0, _lib.PSG_F64)
    yield v
    v.close()


@pytest.fixture(scope="module")
def scalar(ctx):
    w = DarlingWorker(ctx._h, DELTA_INIT, 5.0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def multi(ctx):
    ws = {}

    def get(m):
        if m not in ws:
            ws[m] = DarlingMultiWorker(ctx._h, m, DELTA_INIT, 5.0 + 0.25 * np.arange(m))
        return ws[m]
    yield get
    for w in ws.values():
        w.close()


def state_of(j, special):
    """Model j's state over D.case: its own dual, weights, delta and active
    columns (D.some_inactive's, and three more drawn per model)."""
    rng = np.random.default_rng(300 + j)
    dual = D.special_dual(rng, D.ROWS) if special and j % 2 else D.spread_dual(rng, D.ROWS)
    cur_w = rng.standard_normal(60)
    cur_w[j % 5::5] = 0.0
    active = D.some_inactive(rng, D.column_lens())
    active[rng.choice(60, size=3, replace=False)] = 0
    return dict(dual=dual, cur_w=cur_w, delta=rng.uniform(0.1, 3.0, 60), active=active), rng


def mask_of(states):
    return sum((s["active"].astype(np.uint32) << np.uint32(j)) for j, s in enumerate(states))


def drive(mw, states, nws, cb, ce):
    """set_state, gradients, update_dual, objv on the multi worker: G, U, state, objv."""
    col = lambda name: np.stack([s[name] for s in states], axis=1)  # noqa: E731
    mw.set_state(dual=col("dual"), cur_w=col("cur_w"), delta=col("delta"), mask=mask_of(states))
    G, U = mw.gradients(cb, ce)
    mw.update_dual(cb, ce, np.stack(nws, axis=1))
    return G, U, mw.state(), mw.objv()


# -------------------------------------------------- 1. column identity --
@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("m", MS)
def test_column_is_the_scalar_device_path(multi, scalar, m, binary):
    c = D.case(binary, 1)
    mw = multi(m)
    mw.load(*c)
    scalar.load(*c)
    for cb, ce in RANGES:
        states, nws = [], []
        for j in range(m):
            st, rng = state_of(j, True)
            states.append(st)
            nws.append(D.update_weights(rng, st["cur_w"], cb, ce, mw.delta_max[j]))
        G, U, now, objv = drive(mw, states, nws, cb, ce)
        assert G.shape == (ce - cb, m) and now["delta_w"].shape == (ce - cb, m)
        for j, st in enumerate(states):
            scalar.delta_max = float(mw.delta_max[j])
            scalar.set_state(**st)
            Gs, Us = scalar.gradients(cb, ce)
            scalar.update_dual(cb, ce, nws[j])
            want = scalar.state()
            assert same(G[:, j], Gs) and same(U[:, j], Us), (cb, ce, j)
            off = st["active"][cb:ce] == 0
            assert off.any() and np.all(D.bits(G[:, j])[off] == ONES)
            assert np.all(D.bits(U[:, j])[off] == ONES) and not np.isnan(G[:, j][~off]).any()
            for name in ("dual", "cur_w", "delta", "delta_w"):
                assert same(now[name][:, j], want[name]), (name, cb, ce, j)
            assert same(((now["mask"] >> np.uint32(j)) & 1).astype(np.uint8), want["active"])
            assert same(objv[j:j + 1], np.array([scalar.objv()]))
        if m > 1:
            assert len({s["active"].tobytes() for s in states}) > 1  # the masks differ


# ------------------------------------------- 2. the host's restatement --
@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("m", MS)
def test_column_against_the_host_reference(multi, m, binary):
    c = D.case(binary, 1)
    y, dic = c[3], c[4]
    z = D.localized(c[0], c[1], c[2], dic)
    cols = D.scalar_columns(*z, dic.size)
    lens = D.column_lens()
    mw = multi(m)
    mw.load(*c)
    for cb, ce in RANGES:
        states, nws = [], []
        for j in range(m):
            st, rng = state_of(j, False)
            states.append(st)
            nws.append(D.update_weights(rng, st["cur_w"], cb, ce, mw.delta_max[j]))
        G, U, now, objv = drive(mw, states, nws, cb, ce)
        for j, st in enumerate(states):
            wantG, wantU = D.scalar_gradients(cols, binary, y, st["dual"], st["delta"],
                                              st["active"], cb, ce)
            want = D.scalar_update_dual(cols, binary, y, st["dual"], st["cur_w"], st["delta"],
                                        st["active"], cb, ce, nws[j], mw.delta_max[j])
            assert same(G[:, j], wantG), (cb, ce, j)
            live = st["active"][cb:ce] == 1
            assert np.isfinite(wantU[live]).all() and same(U[:, j][~live], wantU[~live])
            assert within(U[:, j][live], wantU[live], D.u_bound(wantU, lens[cb:ce], binary)[live])
            assert same(now["cur_w"][:, j], want[1]) and same(now["delta"][:, j], want[2])
            assert same(((now["mask"] >> np.uint32(j)) & 1).astype(np.uint8), want[3])
            assert same(now["delta_w"][:, j], want[4])
            nfac = want[5]
            assert same(now["dual"][:, j][nfac == 0], st["dual"][nfac == 0])
            assert within(now["dual"][:, j], want[0], D.dual_bound(want[0], nfac))
            got_dual = now["dual"][:, j]
            assert within(objv[j], D.scalar_objv(got_dual),
                          D.objv_bound(D.scalar_objv_terms(got_dual)))


# ------------------------------------------------- 3. untouched rows --
def test_rows_touched_only_by_idle_columns_of_a_model_keep_its_bits(multi):
    """Models 0 and 2: every column has delta_w == 0 (+0.0 or -0.0) or is
    inactive, so their dual columns keep their bits (a NaN's payload
    included) while model 1 changes the same rows."""
    c = D.case(False)
    mw = multi(3)
    mw.load(*c)
    rng = np.random.default_rng(26)
    dual = np.stack([D.special_dual(rng, D.ROWS) for _ in range(3)], axis=1)
    dual[5, 0] = np.array([0x7FF8000000000ABC], np.uint64).view(np.float64)[0]
    active = D.some_inactive(rng, D.column_lens())
    idle = np.where(rng.random(60) < 0.5, 0.0, -0.0)
    idle[active == 0] = 3.0  # delta_w != 0 on an inactive column
    nw = np.stack([idle, rng.standard_normal(60) * 0.3, idle], axis=1)
    states = [dict(active=active), dict(active=np.ones(60, np.uint8)), dict(active=active)]
    mw.set_state(dual=dual, cur_w=np.zeros((60, 3)), delta=np.ones((60, 3)), mask=mask_of(states))
    mw.update_dual(0, 60, nw)
    st = mw.state()
    assert same(st["dual"][:, 0], dual[:, 0]) and same(st["dual"][:, 2], dual[:, 2])
    changed = D.bits(st["dual"][:, 1]) != D.bits(dual[:, 1])
    assert changed.sum() > D.ROWS // 2
    assert same(st["cur_w"], nw) and same(st["mask"], mask_of(states))


# --------------------------------------------------- 4. server update --
def server_inputs(rng, n, m):
    """Every branch of updateWeight: w = 0 with g_pos < 0, with g_neg > 0 and
    between (inactivated where the threshold is small); w != 0 on both shrink
    branches and on neither; delta below and above |d|; a cleared bit with the
    all-ones NaN in G and U."""
    w = np.where(rng.random((n, m)) < 0.6, 0.0, rng.standard_normal((n, m)))
    G = rng.standard_normal((n, m)) * 1.5
    U = rng.uniform(0.05, 2.0, (n, m))
    delta = rng.uniform(0.05, 3.0, (n, m))
    act = (rng.random((n, m)) < 0.85).astype(np.uint8)
    G[act == 0] = D.INACTIVE
    U[act == 0] = D.INACTIVE
    return w, G, U, delta, act


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("m", MS)
def test_server_update(ctx, n, m):
    import torch
    settings = [dict(eta=0.5 + 0.1 * j, lambda_=0.1 + 0.2 * (j % 4),
                     kkt_filter_threshold=(0.05, 0.4, 1e20)[j % 3], delta_max=1.0 + j)
                for j in range(m)]
    srv = DarlingMultiServer(ctx._h, np.arange(1, n + 1, dtype=np.uint64), settings, DELTA_INIT)
    rng = np.random.default_rng(1000 * n + m)
    w, G, U, delta, act = server_inputs(rng, n, m)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    srv.w.copy_(to(w))
    srv.delta.copy_(to(delta))
    srv.mask.copy_(to(sum(act[:, j].astype(np.uint32) << np.uint32(j)
                          for j in range(m)).view(np.int32)))
    vio = np.zeros(m)
    for call in range(2):  # the second call max-accumulates the violation
        dG, dU = to(G), to(U)
        torch.cuda.synchronize()
        srv.update(0, n, dG.data_ptr(), dU.data_ptr())
        got_w, got_mask, got_vio = srv.weights(), srv.active(), srv.violation()
        got_delta = srv.delta.cpu().numpy()
        for j, s in enumerate(settings):
            w[:, j], delta[:, j], act[:, j], vio[j] = O.darling_update_weight(
                w[:, j], delta[:, j], act[:, j], 0, G[:, j], U[:, j], s["eta"], s["lambda_"],
                s["kkt_filter_threshold"], s["delta_max"], vio[j])
            assert same(got_w[:, j], w[:, j]) and same(got_delta[:, j], delta[:, j]), (call, j)
            assert same(((got_mask >> np.uint32(j)) & 1).astype(np.uint8), act[:, j]), (call, j)
        assert same(got_vio, vio), call
        G = np.where(act == 0, D.INACTIVE, rng.standard_normal((n, m)) * (0.2 if call == 0 else 3))
    if n == 257:
        assert (D.bits(w) == ONES).any() and (vio > 0).all() and (delta[:, 0] == 1.0).any()
    prog = srv.progress()
    live = ~np.isnan(w) & (w != 0)
    assert np.array_equal(prog["nnz_w"], live.sum(0)) and np.array_equal(prog["nnz_active"],
                                                                         act.sum(0))
    want = np.array([s["lambda_"] for s in settings]) * np.where(live, np.abs(w), 0).sum(0)
    # two sums of n non-negative terms, each within n 2^-53 of the exact sum, and one
    # rounded product with lambda on either side
    assert np.all(np.abs(prog["objv"] - want) <= (n + 2) * 2.0 ** -52 * want)
    srv.close()


# ------------------------------------------------------------ 5. pass --
def split_rows(c, parts):
    """D.case's rows in `parts` contiguous pieces, each a case of its own."""
    offset, index, value, y, dic = c
    cut = np.linspace(0, y.size, parts + 1).astype(int)
    out = []
    for a, b in zip(cut[:-1], cut[1:]):
        lo, hi = int(offset[a]), int(offset[b])
        out.append((offset[a:b + 1] - offset[a], index[lo:hi],
                    None if value is None else value[lo:hi], y[a:b], dic))
    return out


@pytest.mark.parametrize("W", (1, 2))
def test_pass(ctx, W):
    m, chl0 = 3, 40 + 8 * W
    parts = split_rows(D.case(False, 1), W)
    dic = parts[0][4]
    blocks = [(int(dic[0]), int(dic[30])), (int(dic[30]), (1 << 64) - 1)]
    settings = [dict(eta=0.8, lambda_=0.5, kkt_filter_threshold=1e20, delta_max=5.0),
                dict(eta=0.6, lambda_=0.2, kkt_filter_threshold=0.05, delta_max=3.0),
                dict(eta=1.0, lambda_=1.5, kkt_filter_threshold=0.5, delta_max=4.0)]
    srv = DarlingMultiServer(ctx._h, dic, settings, DELTA_INIT)
    mws = [DarlingMultiWorker(ctx._h, m, DELTA_INIT, [s["delta_max"] for s in settings])
           for _ in range(W)]
    sws = [DarlingWorker(ctx._h, DELTA_INIT, 5.0) for _ in range(W)]
    try:
        for wk, p in zip(mws, parts):
            wk.load(*p)
        for _ in range(2):
            darling_pass_rows(srv, mws, blocks)
        got_w, got_mask = srv.weights(), srv.active()
        got_objv = [wk.objv() for wk in mws]
        for j, s in enumerate(settings):
            chl = chl0 + j
            ctx.setValue(Message(key=dic, key_channel=chl))
            ctx.set_value_array(chl, np.zeros(dic.size))
            _lib.check(ctx._L.psg_darling_init(ctx._h, chl, DELTA_INIT))
            for wk, p in zip(sws, parts):
                wk.delta_max = s["delta_max"]
                wk.load(*p)
            t = 10
            for _ in range(2):
                t = darling_pass(ctx, sws, chl, t, blocks, s)
            ctx.dev_status()
            sd, sa = np.empty(dic.size), np.empty(dic.size, np.uint8)
            _lib.check(ctx._L.psg_darling_state(ctx._h, chl, 0, dic.size, sd.ctypes.data,
                                                sa.ctypes.data, None))
            assert same(got_w[:, j], ctx.value(chl)), j
            assert same(((got_mask >> np.uint32(j)) & 1).astype(np.uint8), sa), j
            for i, wk in enumerate(sws):
                assert same(got_objv[i][j:j + 1], np.array([wk.objv()])), (i, j)
        assert (got_mask != 7).any() and np.isfinite(got_w).any()
    finally:
        for wk in mws + sws:
            wk.close()
        srv.close()


# ---------------------------------------------------------- 6. errors --
def test_errors(ctx, multi):
    L, ERR = _lib.lib(), _lib.PSG_ERR_ARG
    offset, index, value, y, dic = D.case(False)
    fresh = Minibatch(ctx._h)
    one = np.zeros(64)
    p = one.ctypes.data  # never read: every call below fails its argument check
    fresh.load(offset, index, value, y)
    fresh.uniq()
    fresh.localize(multi(1)._upload(0, dic), dic.size)
    n = C.c_size_t()
    for m in (0, 33, -1):
        assert L.psg_mb_darling_rows_init(fresh._h, m, 1.0, None, None) == ERR
    assert L.psg_mb_darling_rows_gradients(fresh._h, 0, 1, p, p, None) == ERR  # before the init
    assert L.psg_mb_darling_rows_update_dual(fresh._h, 0, 1, p, p, None) == ERR
    assert L.psg_mb_darling_rows_objv(fresh._h, p, None) == ERR
    assert L.psg_mb_darling_rows_reset_active(fresh._h, None) == ERR
    assert L.psg_mb_rows_read(fresh._h, _lib.PSG_MB_ROWS_DARLING_DUAL, None, 0, C.byref(n)) == ERR
    _lib.check(L.psg_mb_darling_rows_init(fresh._h, 3, 1.0, None, None))
    assert L.psg_mb_darling_rows_gradients(fresh._h, 5, 4, p, p, None) == ERR  # cb > ce
    assert L.psg_mb_darling_rows_gradients(fresh._h, 0, dic.size + 1, p, p, None) == ERR
    assert L.psg_mb_darling_rows_update_dual(fresh._h, 0, dic.size + 1, p, p, None) == ERR
    assert L.psg_mb_darling_rows_set_state(fresh._h, 2, None, None, None, None) == ERR  # wrong m
    bad = np.full(dic.size, 8, np.uint32)  # bit 3 of a state of three models
    assert L.psg_mb_darling_rows_set_state(fresh._h, 3, None, None, None, bad.ctypes.data) == ERR
    v = C.c_double()
    assert L.psg_mb_darling_objv(fresh._h, C.byref(v), None) == ERR  # the scalar state is another
    fresh.load(offset, index, value, y)  # a new load invalidates the state
    assert L.psg_mb_darling_rows_objv(fresh._h, p, None) == ERR
    fresh.close()
    assert L.psg_darling_rows_update_dev(ctx._h, p, p, p, p, p, 1, 33, p, p, None) == ERR
