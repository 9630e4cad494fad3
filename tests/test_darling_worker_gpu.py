"""GPU: the device Darling worker (psg_mb_darling_*, DarlingWorker) against the
restatement in tests/darling_worker_ref.py.

G, cur_w, delta, delta_w and the active bytes hold no exp and are compared bit
for bit; so is U where every term saturates, and dual where nothing touches
it.  U, dual and objv otherwise carry the device's exp / log, and are held to
bounds that are derived, not measured (darling_worker_ref.py, "bounds"): each
side's exp / log is within 1 ulp of the true value, so two results differ by
at most 2 x 2^-52 relatively, and every rounded operation after that adds
2^-53 per side:

  U     (c + n_k) 2^-52 U per column of n_k terms, c = 4 binary, 6 valued
  dual  4 n_i 2^-52 dual per row of n_i factors
  init  2 x 2^-52 dual (one exp of the same argument)
  objv  (rows + 1) 2^-53 objv for the reduction + 2 x 2^-52 x each row's term

The largest fraction of each bound seen on an MI355X is recorded in DESIGN.md
section 7.  One context, one server and one worker handle serve the module;
the seam case has a worker of its own, which it closes."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import darling_worker_ref as D
import oracle_py as O
from parameter_server_amd import DarlingWorker, _lib
from parameter_server_amd.kv_vector import KVVector, Message
from parameter_server_amd.worker import Minibatch

pytestmark = pytest.mark.gpu

DELTA_INIT, DELTA_MAX = 1.0, 5.0
RANGES = ((0, 60), D.INNER, (9, 9), (3, 4), (59, 60))
ONES = 0xFFFFFFFFFFFFFFFF


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return b.dtype == np.float64 and a.shape == b.shape and \
            np.array_equal(D.bits(a), D.bits(b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def within(got, want, bound):
    """Every item equal (infinities included), NaN on both sides, or inside
    its bound; the largest fraction of a bound used, for the record."""
    got, want, bound = np.asarray(got), np.asarray(want), np.asarray(bound)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        ok = both_nan | (got == want) | (err <= bound)
        frac = np.where(both_nan | (got == want) | ~(bound > 0) | ~np.isfinite(bound), 0.0,
                        err / bound)
    return bool(np.all(ok)), float(np.max(frac)) if frac.size else 0.0


@pytest.fixture(scope="module")
def server():
    v = KVVector(0, _lib.PSG_F64)
    yield v
    v.close()


@pytest.fixture(scope="module")
def worker(server):
    w = DarlingWorker(server._h, DELTA_INIT, DELTA_MAX)
    yield w
    w.close()


@functools.lru_cache(maxsize=None)
def case(binary, emax=20):
    offset, index, value, y, dic = D.case(binary, emax)
    return (offset, index, value, y, dic), D.localized(offset, index, value, dic)


def load(worker, binary, emax=20, w=None):
    c, z = case(binary, emax)
    worker.load(*c, w=w)
    return c[3], c[4], z


# ---------------------------------------------------------------- init --
@pytest.mark.parametrize("binary", (False, True))
def test_init_without_weights(worker, binary):
    y, dic, z = load(worker, binary)
    st = worker.state()
    assert same(st["dual"], np.ones(D.ROWS))  # exactly 1.0
    assert same(st["cur_w"], np.zeros(dic.size))
    assert same(st["delta"], np.full(dic.size, DELTA_INIT))
    assert same(st["active"], np.ones(dic.size, np.uint8))
    assert st["delta_w"].size == 0
    got = worker.objv()
    terms = D.scalar_objv_terms(st["dual"])
    ok, frac = within(got, math.fsum(terms), D.objv_bound(terms))
    print("objv of dual = 1: %.3g of its bound" % frac)
    assert ok


@pytest.mark.parametrize("binary", (False, True))
def test_init_from_weights_and_objv(worker, binary):
    """dual = exp(y .* Xw): Xw is bit for bit the host's (psg_mb_times), so
    init_bound; then objv of that dual, and of a dual spread over e^+-15."""
    import worker_ref as R
    c, z = case(binary, 1)
    rng = np.random.default_rng(21)
    w = rng.standard_normal(c[4].size) * 0.5
    y, dic, z = load(worker, binary, 1, w=w)
    st = worker.state()
    assert same(st["cur_w"], w)
    xw = R.vector_times(z[0], z[1], z[2], w)
    want = D.vector_init_dual(y, xw)
    assert np.abs(y * xw).max() > 3 and np.isfinite(want).all() and want.min() > 1e-300
    ok, frac = within(st["dual"], want, D.init_bound(want))
    print("init from w: %.3f of the bound" % frac)
    assert ok
    assert same(st["dual"][[0, -1]], np.ones(2))  # the empty rows: exp(y * +0.0)
    for name, dual in (("init", st["dual"]), ("spread", D.spread_dual(rng, D.ROWS))):
        worker.set_state(dual=dual)
        got = worker.objv()
        terms = D.scalar_objv_terms(dual)
        ok, frac = within(got, math.fsum(terms), D.objv_bound(terms))
        print("objv (%s dual): %.3g of its bound" % (name, frac))
        assert ok
        assert D.bits(np.array([worker.objv()]))[0] == D.bits(np.array([got]))[0]


# ----------------------------------------------------------- gradients --
@pytest.mark.parametrize("binary", (False, True))
def test_G_bit_exact_with_special_dual(worker, binary):
    """G holds no exp.  dual holds 0, +inf, denormals and e^+-15; some columns
    of every kind of length are inactive; every range of RANGES."""
    y, dic, z = load(worker, binary)
    rng = np.random.default_rng(22)
    lens = D.column_lens()
    dual, delta = D.special_dual(rng, D.ROWS), rng.uniform(0.1, 3.0, dic.size)
    for active in (np.ones(dic.size, np.uint8), D.some_inactive(rng, lens)):
        worker.set_state(dual=dual, delta=delta, active=active)
        for cb, ce in RANGES:
            G, U = worker.gradients(cb, ce)
            wantG, wantU = D.vector_gradients(*z, dic.size, y, dual, delta, active, cb, ce)
            assert G.size == ce - cb and U.size == ce - cb
            assert same(G, wantG), (cb, ce)
            off = active[cb:ce] == 0
            assert np.all(D.bits(G)[off] == ONES) and np.all(D.bits(U)[off] == ONES)
            empty = (lens[cb:ce] == 0) & ~off
            assert not D.bits(G)[empty].any() and not D.bits(U)[empty].any()  # +0.0
            assert np.array_equal(np.isnan(U), np.isnan(wantU))
    assert (active == 0).sum() >= 4 and (lens == 0).sum() >= 3


@pytest.mark.parametrize("binary", (False, True))
def test_U_bit_exact_when_saturated(worker, binary):
    """delta = 5, dual in [1/2, 2]: tau (1 - tau) >= 2/9 and exp(|v| delta) >=
    exp(5 x 2^-5), so every term is exactly .25 (or .25 v v) whatever exp
    returns within an ulp: U checks the sum's order alone."""
    y, dic, z = load(worker, binary)
    rng = np.random.default_rng(23)
    dual, delta = np.exp2(rng.uniform(-1, 1, D.ROWS)), np.full(dic.size, 5.0)
    worker.set_state(dual=dual, delta=delta, active=np.ones(dic.size, np.uint8))
    for cb, ce in RANGES:
        G, U = worker.gradients(cb, ce)
        wantG, wantU = D.vector_gradients(*z, dic.size, y, dual, delta, np.ones(dic.size), cb, ce)
        assert same(U, wantU) and same(G, wantG), (cb, ce)


@pytest.mark.parametrize("binary", (False, True))
def test_U_within_bound(worker, binary):
    y, dic, z = load(worker, binary, 1)
    rng = np.random.default_rng(24)
    dual, delta = D.spread_dual(rng, D.ROWS), rng.uniform(0.1, 3.0, dic.size)
    active = D.some_inactive(rng, D.column_lens())
    worker.set_state(dual=dual, delta=delta, active=active)
    G, U = worker.gradients(0, dic.size)
    wantG, wantU = D.vector_gradients(*z, dic.size, y, dual, delta, active, 0, dic.size)
    assert same(G, wantG)
    live = active == 1
    assert np.isfinite(wantU[live]).all()
    ok, frac = within(U[live], wantU[live], D.u_bound(wantU, D.column_lens(), binary)[live])
    # not every term may saturate, or this checks nothing the test above does not
    _, sat = D.vector_gradients(*z, dic.size, y, np.ones(D.ROWS), np.full(dic.size, 5.0), active,
                                0, dic.size)
    assert np.mean(wantU[live] < sat[live]) > 0.5
    print("U: %.3f of its bound" % frac)
    assert ok


# --------------------------------------------------------- update_dual --
@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("rng_", ((0, 60), D.INNER))
def test_update_dual(worker, binary, rng_):
    cb, ce = rng_
    y, dic, z = load(worker, binary, 1)
    rng = np.random.default_rng(25)
    dual = D.spread_dual(rng, D.ROWS)
    cur_w = rng.standard_normal(dic.size)
    cur_w[::5] = 0.0
    delta = rng.uniform(0.1, 3.0, dic.size)
    active = D.some_inactive(rng, D.column_lens())
    nw = D.update_weights(rng, cur_w, cb, ce, DELTA_MAX)
    assert np.any(D.bits(nw) == ONES) and np.any(np.isnan(nw) & (D.bits(nw) != ONES))
    assert np.any(D.bits(nw) == 1 << 63) and np.any(nw == cur_w[cb:ce])
    want = D.vector_update_dual(*z, dic.size, y, dual, cur_w, delta, active, cb, ce, nw, DELTA_MAX)
    assert np.any(want[2] == DELTA_MAX) and want[3].sum() < active.sum()
    worker.set_state(dual=dual, cur_w=cur_w, delta=delta, active=active)
    worker.update_dual(cb, ce, nw)
    st = worker.state()
    assert same(st["cur_w"], want[1]) and same(st["delta"], want[2])
    assert same(st["active"], want[3]) and same(st["delta_w"], want[4])
    nfac = want[5]
    untouched = nfac == 0
    assert untouched.sum() >= 2 and same(st["dual"][untouched], dual[untouched])
    assert want[0][~untouched].min() > 1e-300
    ok, frac = within(st["dual"], want[0], D.dual_bound(want[0], nfac))
    print("dual after update of [%d, %d): %.3f of its bound, up to %d factors"
          % (cb, ce, frac, nfac.max()))
    assert ok


def test_rows_touched_only_by_idle_columns_keep_their_bits(worker):
    """Every column either has delta_w == 0 (+0.0 or -0.0) or is inactive:
    no dual changes, whatever its bits (a NaN's payload included)."""
    y, dic, z = load(worker, False)
    rng = np.random.default_rng(26)
    dual = D.special_dual(rng, D.ROWS)
    dual[5] = np.array([0x7FF8000000000ABC], np.uint64).view(np.float64)[0]
    cur_w = np.zeros(dic.size)
    active = D.some_inactive(rng, D.column_lens())
    nw = np.where(rng.random(dic.size) < 0.5, 0.0, -0.0)
    nw[active == 0] = 3.0  # delta_w != 0 on an inactive column
    worker.set_state(dual=dual, cur_w=cur_w, delta=np.ones(dic.size), active=active)
    worker.update_dual(0, dic.size, nw)
    st = worker.state()
    assert same(st["dual"], dual)
    assert same(st["cur_w"], nw) and same(st["active"], active)


@pytest.mark.parametrize("binary", (False, True))
def test_repeatable(worker, binary):
    y, dic, z = load(worker, binary, 1)
    rng = np.random.default_rng(27)
    state = dict(dual=D.spread_dual(rng, D.ROWS), cur_w=rng.standard_normal(dic.size),
                 delta=rng.uniform(0.1, 3.0, dic.size), active=np.ones(dic.size, np.uint8))
    nw = state["cur_w"] + rng.standard_normal(dic.size) * 2.0 ** -3
    runs = []
    for _ in range(2):
        worker.set_state(**state)
        G, U = worker.gradients(0, dic.size)
        worker.update_dual(0, dic.size, nw)
        runs.append((G, U, worker.state()["dual"], np.array([worker.objv()])))
    for a, b in zip(*runs):
        assert same(a, b)


# ------------------------------------------------------- the seam case --
def test_seam_case(server):
    """worker_ref.seam_case's structure with this worker's values (what it
    reaches: tests/test_worker.py): more long columns than
    darling_sum_long_kernel has waves, a column at every edge of the short /
    long split and of a chain_sum2 batch, more than 65,536 rows (three digit
    passes of the sort by row, objv_kernel's second trip), more than 256
    tiles in every scan.  Init from weights, gradients over three blocks, one
    update_dual with update_weights' special values, the objective; twice
    from one state."""
    import worker_ref as R
    from parameter_server_amd.worker import sort_tile
    offset, index, value, y, dic = D.seam_case(sort_tile())
    z = D.localized(offset, index, value, dic)
    nd, rows = dic.size, y.size
    lens = np.bincount(z[1].astype(np.int64), minlength=nd)
    assert rows > 65536 and (lens > R.LONG_RUN).sum() > 4 * R.LONG_GRID
    assert set(R.SEAM_EDGE_RUNS) <= set(lens.tolist())
    assert {2 * R.CHAIN2 - 1, 2 * R.CHAIN2, 2 * R.CHAIN2 + 1, 4 * R.CHAIN2,
            4 * R.CHAIN2 + 1} <= set(R.SEAM_EDGE_RUNS)  # whole batches of chain_sum2, and one over
    rng = np.random.default_rng(71)
    w = rng.standard_normal(nd) * 0.5
    third = (nd // 3, 2 * nd // 3)
    one = int(np.nonzero(lens == 2 * R.CHAIN + 1)[0][0])
    blocks = ((0, nd), third, (one, one + 1))
    delta = rng.uniform(0.1, 3.0, nd)
    active = np.ones(nd, np.uint8)
    active[rng.choice(nd, size=nd // 50, replace=False)] = 0
    active[one] = 1
    big = DarlingWorker(server._h, DELTA_INIT, DELTA_MAX)
    try:
        big.load(offset, index, value, y, dic, w=w)
        st = big.state()
        # init: Xw is bit for bit the host's, then one exp
        assert same(st["cur_w"], w) and same(st["delta"], np.full(nd, DELTA_INIT))
        xw = R.vector_times(z[0], z[1], z[2], w)
        want_dual = D.vector_init_dual(y, xw)
        assert np.abs(y * xw).max() > 3 and np.isfinite(want_dual).all() and \
            want_dual.min() > 1e-300
        ok, f_init = within(st["dual"], want_dual, D.init_bound(want_dual))
        assert ok
        assert same(st["dual"][[0, 7, 8, -1]], np.ones(4))  # the empty rows
        # from here on both sides start from the device's own dual
        dual = st["dual"]
        wantG, wantU = D.vector_gradients(*z, nd, y, dual, delta, active, 0, nd)
        nw = D.update_weights(rng, w, *third, DELTA_MAX)
        want = D.vector_update_dual(*z, nd, y, dual, w, delta, active, *third, nw, DELTA_MAX)
        nfac = want[5]
        assert (nfac == 0).sum() >= 4 and nfac.max() >= 4
        assert np.isfinite(want[0]).all() and want[0].min() > 1e-300
        assert np.isfinite(wantU[active == 1]).all()
        runs = []
        for _ in range(2):
            big.set_state(dual=dual, cur_w=w, delta=delta, active=active)
            got = [big.gradients(cb, ce) for cb, ce in blocks]
            big.update_dual(*third, nw)
            now = big.state()
            runs.append(got + [now["dual"], np.array([big.objv()])])
        f_u = 0.0
        for (cb, ce), (G, U) in zip(blocks, runs[0][:3]):
            assert G.size == ce - cb and same(G, wantG[cb:ce]), (cb, ce)
            live = active[cb:ce] == 1
            assert np.all(D.bits(U)[~live] == ONES) and np.all(D.bits(G)[~live] == ONES)
            ok, f = within(U[live], wantU[cb:ce][live],
                           D.u_bound(wantU[cb:ce], lens[cb:ce], False)[live])
            assert ok, (cb, ce)
            f_u = max(f_u, f)
        assert same(now["cur_w"], want[1]) and same(now["delta"], want[2])
        assert same(now["active"], want[3]) and same(now["delta_w"], want[4])
        assert same(now["dual"][nfac == 0], dual[nfac == 0])
        ok, f_dual = within(now["dual"], want[0], D.dual_bound(want[0], nfac))
        assert ok
        terms = D.scalar_objv_terms(now["dual"])
        ok, f_objv = within(runs[0][4][0], math.fsum(terms), D.objv_bound(terms))
        assert ok
        print("seam case: init %.3f, U %.3f, dual %.3f (up to %d factors), objv %.3g of their "
              "bounds" % (f_init, f_u, f_dual, nfac.max(), f_objv))
        for a, b in zip(runs[0][:3], runs[1][:3]):
            assert same(a[0], b[0]) and same(a[1], b[1])
        assert same(runs[0][3], runs[1][3]) and same(runs[0][4], runs[1][4])
    finally:
        big.close()


# ------------------------------------------ the sort by row's pass count --
@pytest.mark.parametrize("rows", D.ROW_COUNTS)
def test_row_sort_pass_counts(worker, rows):
    """255, 256, 65,535 and 65,536 rows: 1, 2, 2 and 3 digit passes, so the
    rows' lists end on either side of the sort's two buffers.  The cases tell
    a wrong order of a row's factors (tests/test_darling_worker.py)."""
    offset, index, value, y, dic = D.row_case(rows)
    z = D.localized(offset, index, value, dic)
    dual, cur_w, delta, active, nw = D.row_case_update(rows)
    want = D.vector_update_dual(*z, dic.size, y, dual, cur_w, delta, active, 0, dic.size, nw,
                                DELTA_MAX)
    worker.load(offset, index, value, y, dic)
    worker.set_state(dual=dual, cur_w=cur_w, delta=delta, active=active)
    worker.update_dual(0, dic.size, nw)
    st = worker.state()
    nfac = want[5]
    assert nfac[0] == nfac[rows // 2] == nfac[-1] == 12
    assert same(st["dual"][nfac == 0], dual[nfac == 0])
    ok, frac = within(st["dual"], want[0], D.dual_bound(want[0], nfac))
    print("rows %d: dual %.3f of its bound" % (rows, frac))
    assert ok
    assert same(st["cur_w"], want[1]) and same(st["delta_w"], want[4])


# ------------------------------------------------------------ lockstep --
def test_lockstep_with_the_server(server, worker):
    """block_step against the KVVector server, 3 blocks x 2 passes, the second
    with a KKT threshold that deactivates columns.  Before each block the
    device's state is read and the restatement takes that one block from it,
    with the oracle's updateWeight on the device's own (G, U) as the server:
    ulp noise cannot flip a branch further down."""
    binary, chl = False, 3
    y, dic, z = load(worker, binary, 1)
    server.setValue(Message(key=dic, key_channel=chl))
    server.set_value_array(chl, np.zeros(dic.size))
    _lib.check(server._L.psg_darling_init(server._h, chl, DELTA_INIT))
    eta, lam = 0.8, 0.5
    t, fracs, dropped = 10, [0.0, 0.0], 0
    for it in range(2):
        kkt = 1e20 if it == 0 else 0.05
        for cb, ce in ((0, 9), (9, 31), (31, 60)):
            st = worker.state()
            sw = server.value(chl)
            sd, sa = np.empty(dic.size), np.empty(dic.size, np.uint8)
            _lib.check(server._L.psg_darling_state(server._h, chl, 0, dic.size, sd.ctypes.data,
                                                   sa.ctypes.data, None))
            assert same(sa, st["active"])  # the worker's view of the active set is the server's
            G, U = worker.gradients(cb, ce)
            wantG, wantU = D.vector_gradients(*z, dic.size, y, st["dual"], st["delta"],
                                              st["active"], cb, ce)
            assert same(G, wantG)
            live = st["active"][cb:ce] == 1
            ok, f = within(U[live], wantU[live],
                           D.u_bound(wantU, D.column_lens()[cb:ce], binary)[live])
            assert ok and same(U[~live], wantU[~live])
            fracs[0] = max(fracs[0], f)
            w2, d2, a2, vio_o = O.darling_update_weight(sw, sd, sa, cb, G, U, eta, lam, kkt,
                                                        DELTA_MAX, 0.0)
            vio = worker.block_step(server, chl, t, cb, ce,
                                    dict(eta=eta, lambda_=lam, kkt_filter_threshold=kkt))
            assert vio == vio_o and same(server.value(chl), w2)
            want = D.vector_update_dual(*z, dic.size, y, st["dual"], st["cur_w"], st["delta"],
                                        st["active"], cb, ce, w2[cb:ce], DELTA_MAX)
            now = worker.state()
            assert same(now["cur_w"], want[1]) and same(now["delta"], want[2])
            assert same(now["active"], want[3]) and same(now["delta_w"], want[4])
            assert np.isfinite(want[0]).all() and want[0].min() > 1e-300
            ok, f = within(now["dual"], want[0], D.dual_bound(want[0], want[5]))
            assert ok
            fracs[1] = max(fracs[1], f)
            dropped += int(st["active"].sum()) - int(now["active"].sum())
            t += 3
    print("lockstep: U %.3f, dual %.3f of their bounds; %d columns deactivated"
          % (fracs[0], fracs[1], dropped))
    assert dropped > 0
    worker.reset_active()
    assert worker.state()["active"].all()


# -------------------------------------------------------------- errors --
def test_errors(server, worker):
    L, ERR = _lib.lib(), _lib.PSG_ERR_ARG
    c, z = case(False)
    offset, index, value, y, dic = c
    fresh = Minibatch(server._h)
    n, v = C.c_size_t(), C.c_double()
    one = np.zeros(8)
    p = one.ctypes.data  # never read: every call below fails its argument check
    assert L.psg_mb_darling_init(fresh._h, 1.0, None, None) == ERR  # before load
    fresh.load(offset, index, value, y)
    fresh.uniq()
    assert L.psg_mb_darling_init(fresh._h, 1.0, None, None) == ERR  # before localize
    d = worker._upload(worker._DICT, dic)
    fresh.localize(d, dic.size)
    assert L.psg_mb_darling_gradients(fresh._h, 0, 1, p, p, None) == ERR  # before init
    assert L.psg_mb_darling_update_dual(fresh._h, 0, 1, p, 5.0, None) == ERR
    assert L.psg_mb_darling_objv(fresh._h, C.byref(v), None) == ERR
    assert L.psg_mb_darling_reset_active(fresh._h, None) == ERR
    assert L.psg_mb_darling_set_state(fresh._h, None, None, None, None) == ERR
    assert L.psg_mb_read(fresh._h, _lib.PSG_MB_DARLING_DUAL, None, 0, C.byref(n)) == ERR
    _lib.check(L.psg_mb_darling_init(fresh._h, 1.0, None, None))
    assert L.psg_mb_darling_gradients(fresh._h, 0, dic.size + 1, p, p, None) == ERR  # ce > ndict
    assert L.psg_mb_darling_update_dual(fresh._h, 0, dic.size + 1, p, 5.0, None) == ERR
    assert L.psg_mb_darling_gradients(fresh._h, 5, 4, p, p, None) == ERR  # cb > ce
    assert L.psg_mb_darling_gradients(fresh._h, 0, 1, None, None, None) == ERR
    bad = np.full(dic.size, 2, np.uint8)
    assert L.psg_mb_darling_set_state(fresh._h, None, None, None, bad.ctypes.data) == ERR
    assert L.psg_mb_read(fresh._h, _lib.PSG_MB_DARLING_DUAL, None, 0, C.byref(n)) == \
        _lib.PSG_ERR_SIZE and n.value == D.ROWS
    fresh.load(offset, index, value, y)  # a new load invalidates the state
    assert L.psg_mb_darling_objv(fresh._h, C.byref(v), None) == ERR
    fresh.uniq()
    fresh.localize(d, dic.size)  # ... and so does a new localize
    assert L.psg_mb_darling_objv(fresh._h, C.byref(v), None) == ERR
    _lib.check(L.psg_mb_darling_init(fresh._h, 1.0, None, None))
    _lib.check(L.psg_mb_darling_objv(fresh._h, C.byref(v), None))
    assert abs(v.value - D.ROWS * math.log(2.0)) <= D.ROWS * 2.0 ** -50
    fresh.close()
    h32 = C.c_void_p()  # an F32 context has no minibatch, so no Darling worker
    _lib.check(L.psg_create(0, _lib.PSG_F32, 0, C.byref(h32)))
    with pytest.raises(_lib.PSGError) as e:
        DarlingWorker(h32, 1.0, 5.0)
    assert e.value.status == ERR
    L.psg_destroy(h32)
