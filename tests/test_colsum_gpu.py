"""GPU: the product entries in blocked order (psg_mb_set_sum_order) against B
of the terms, restated in tests/test_colsum.py, bit for bit.  The terms are
formed on the host from the same arrays (one rounded product each), or read
back where the device's exp made them (Darling).

Level 3 (a run past 4096^2 terms) is not run on the device: it is one more
trip of the launch loop that level 2 takes, and the host twin covers its
arithmetic (test_colsum.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import worker_ref as R
from parameter_server_amd import _lib
from parameter_server_amd.darling import DarlingWorker
from parameter_server_amd.worker import Minibatch
from test_colsum import LENGTHS, blocked_sum

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning")]
KEY = 1 << 40  # the key of the run under test: fillers lie on both sides of it


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    return t if t.numel() else torch.zeros(8, dtype=torch.uint8, device="cuda:0")


@pytest.fixture(scope="module")
def ctx():
    h = C.c_void_p()
    _lib.check(_lib.lib().psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    yield h
    _lib.lib().psg_destroy(h)


@pytest.fixture(scope="module")
def mb(ctx):
    m = Minibatch(ctx)
    m.set_sum_order("blocked")
    yield m
    m.close()


def build(runs, seed, binary=False, fillers=300, first=0):
    """A minibatch holding key KEY + i with a run of runs[i], its pairs in
    consecutive rows from `first` on, and `fillers` keys with runs 1 .. 40 at
    random rows; the dictionary drops every 7th filler and has two absent keys."""
    rng = np.random.default_rng(seed)
    rows = max(max(runs), 50) + first
    fill = rng.permutation(np.concatenate([np.arange(1, fillers // 2 + 1) * 3,
                                           KEY + 10 ** 6 + np.arange(fillers - fillers // 2) * 5]))
    keys = np.concatenate([KEY + np.arange(len(runs)), fill]).astype(np.uint64)
    lens = np.concatenate([runs, 1 + np.arange(fillers) % 40]).astype(np.int64)
    start = np.concatenate([np.full(len(runs), first), rng.integers(0, rows, fillers)])
    index = np.repeat(keys, lens)
    row = (np.repeat(start, lens) + np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)) % rows
    order = np.argsort(row, kind="stable")
    offset = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=rows))]).astype(np.uint64)
    value = None if binary else R.sensitive_values(rng, index.size)
    dic = np.sort(np.concatenate([keys[:len(runs)], np.delete(fill, np.s_[::7]),
                                  [2, KEY + 7 * 10 ** 7]]).astype(np.uint64))
    return offset, index[order], value, rng.choice([1.0, -1.0], rows), dic


def runs_of(index, dic):  # the sorted pairs' order, every dictionary key's run [lo, hi) in it
    order = np.argsort(index, kind="stable")
    return order, np.searchsorted(index[order], dic, "left"), np.searchsorted(index[order], dic, "right")


def want_sums(offset, index, value, c, dic, fold=blocked_sum):
    row = np.repeat(np.arange(offset.size - 1), np.diff(offset.astype(np.int64)))
    order, lo, hi = runs_of(index, dic)
    t = (c[row] if value is None else c[row] * value)[order]
    return np.array([fold(t[a:b]) for a, b in zip(lo, hi)])


def load(mb, case):
    offset, index, value, y, dic = case
    mb.load(offset, index, value, y)
    mb.uniq()
    d = dev(dic)
    mb.localize(d.data_ptr(), dic.size)
    mb.read("pos")  # waits: d may go
    return R.sensitive_values(np.random.default_rng(index.size), offset.size - 1)


def trans_times(mb, c, ndict):
    cd, g = dev(c), torch.empty(ndict, dtype=torch.float64, device="cuda:0")
    mb.trans_times(cd.data_ptr(), g.data_ptr())
    mb.read("pos")  # waits
    return g.cpu().numpy()


@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("run", LENGTHS[:-1])
def test_trans_times_is_B_of_the_terms(mb, run, binary):
    case = build([run], run + 1, binary)
    c = load(mb, case)
    assert np.array_equal(bits(trans_times(mb, c, case[4].size)), bits(want_sums(*case[:3], c, case[4])))


def test_many_long_and_several_huge_runs_share_the_tables(mb):
    """More long runs than waves of one launch, and three huge runs."""
    case = build(np.concatenate([33 + np.arange(4200) % 15, [4097, 8193, 12289]]), 5)
    c = load(mb, case)
    assert np.array_equal(bits(trans_times(mb, c, case[4].size)), bits(want_sums(*case[:3], c, case[4])))


GRAD_RUNS = [32, 33, 64, 65, 4096, 4097, 2 * 4096 + 1]


@pytest.mark.parametrize("m", (0, 1, 3, 32))  # 0: psg_mb_gradient
def test_gradient_is_B_of_its_terms(mb, m):
    offset, index, value, y, dic = case = build(GRAD_RUNS, 11)
    load(mb, case)
    w = dev(0.1 * np.random.default_rng(m).standard_normal(dic.size * max(m, 1)))
    if m == 0:
        mb.gradient(w.data_ptr())
        tau, got = mb.read("tau").reshape(-1, 1), mb.read("grad").reshape(-1, 1)
    else:
        mb.gradient_rows(w.data_ptr(), m)
        tau, got = mb.read_rows("tau"), mb.read_rows("grad")
    for j in range(max(m, 1)):
        want = want_sums(offset, index, value, -y * tau[:, j], dic)
        assert np.array_equal(bits(got[:, j]), bits(want)), j


def test_darling_gradients_are_B_of_the_term_pairs(ctx):
    offset, index, value, y, dic = build(GRAD_RUNS, 13)
    wk = DarlingWorker(ctx, 1.0, 5.0, sum_order="blocked")
    wk.load(offset, index, value, y, dic, 0.1 * np.random.default_rng(2).standard_normal(dic.size))
    active = np.ones(dic.size, np.uint8)
    off = int(np.searchsorted(dic, KEY + 4))  # the run of 4096: inactive
    active[off] = 0
    wk.set_state(active=active)
    cb, ce = 3, dic.size  # every run of GRAD_RUNS, and the absent key KEY + 7e7 (empty) last
    g, u = wk.gradients(cb, ce)
    t = wk.mb._read(_lib.PSG_MB_DARLING_TERMS, np.float64).reshape(-1, 2)
    _, lo, hi = runs_of(index, dic)
    for k in range(cb, ce):
        if k == off:  # its terms are not written
            assert bits(g[k - cb]) == bits(u[k - cb]) == 0xFFFFFFFFFFFFFFFF
            continue
        want = [blocked_sum(t[lo[k]:hi[k], j]) for j in (0, 1)]
        assert (bits(g[k - cb]), bits(u[k - cb])) == (bits(want[0]), bits(want[1])), k
    assert lo[ce - 1] == hi[ce - 1] and bits(g[-1]) == bits(u[-1]) == 0  # the empty column: +0.0
    wk.close()


def test_switching_orders_on_one_handle(mb):
    offset, index, value, y, dic = case = build([32, 33, 5000], 17)
    c = load(mb, case)
    first = trans_times(mb, c, dic.size)
    mb.set_sum_order("reference")
    ref = trans_times(mb, c, dic.size)
    assert mb.sum_order == "reference"
    mb.set_sum_order("blocked")
    again = trans_times(mb, c, dic.size)
    z = [mb.read(n) for n in ("new_offset", "new_index", "new_value")]
    assert np.array_equal(bits(ref), bits(R.vector_trans_times(*z, c, dic.size)))
    assert np.array_equal(bits(first), bits(again))
    assert np.array_equal(bits(first), bits(want_sums(offset, index, value, c, dic)))
    short = np.searchsorted(dic, KEY)  # the run of exactly 32
    assert bits(first)[short] == bits(ref)[short]
    assert np.any(bits(first) != bits(ref))


@pytest.mark.parametrize("run", (100, 4096, 3 * 4096 + 9))
def test_a_run_gives_the_same_bits_wherever_it_lies(mb, run):
    got = []
    c_run = R.sensitive_values(np.random.default_rng(run), run)
    for first, fillers in ((0, 40), (37, 300)):
        case = build([run], first + 1, binary=True, fillers=fillers, first=first)
        c = load(mb, case)
        c[first:first + run] = c_run
        got.append(trans_times(mb, c, case[4].size)[np.searchsorted(case[4], KEY)])
    assert bits(got[0]) == bits(got[1]) == bits(blocked_sum(c_run))
