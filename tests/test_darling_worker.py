"""CPU: the two restatements of the Darling worker (tests/darling_worker_ref.py)
agree bit for bit on every case the GPU tests use, and the cases can tell a
wrong summation order from the right one."""
import numpy as np
import pytest

import darling_worker_ref as D

DELTA_MAX = 5.0


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return b.dtype == np.float64 and a.shape == b.shape and \
            np.array_equal(D.bits(a), D.bits(b))
    return a.shape == b.shape and np.array_equal(a, b)


def build(binary, emax=20):
    offset, index, value, y, dic = D.case(binary, emax)
    z = D.localized(offset, index, value, dic)
    return z, y, dic, D.scalar_columns(*z, dic.size)


RANGES = ((0, 60), D.INNER, (9, 9), (3, 4), (59, 60))


@pytest.mark.parametrize("binary", (False, True))
def test_case_has_every_column_length(binary):
    offset, index, value, y, dic = D.case(binary)
    z, lens = D.localized(offset, index, value, dic), D.column_lens()
    assert offset.size == D.ROWS + 1 and dic.size == 60 and np.all(np.diff(dic.astype(object)) > 0)
    got = np.bincount(z[1].astype(np.int64), minlength=dic.size)
    assert np.array_equal(got, lens)
    assert set(lens.tolist()) >= {0, 1, 32, 33, 64, 200, 512, 513, 700}
    assert np.sum(lens == 0) >= 2 and np.sum(~np.isin(np.unique(index), dic)) >= 1
    off = offset.astype(np.int64)
    assert off[1] == 0 and off[-1] == off[-2]  # rows 0 and ROWS - 1 are empty
    side_by_side = index[1:] == index[:-1]
    row = np.repeat(np.arange(D.ROWS), np.diff(off))
    assert np.any(side_by_side & (row[1:] == row[:-1]))  # a column twice in a row, adjacent
    if not binary:
        assert np.abs(value).min() >= 2.0 ** -5


@pytest.mark.parametrize("binary", (False, True))
def test_forms_agree_on_gradients(binary):
    z, y, dic, cols = build(binary)
    rng = np.random.default_rng(5)
    for dual in (D.special_dual(rng, D.ROWS), D.spread_dual(rng, D.ROWS),
                 np.exp2(rng.uniform(-1, 1, D.ROWS))):
        for delta in (np.full(dic.size, 5.0), rng.uniform(0.1, 3.0, dic.size)):
            for active in (np.ones(dic.size, np.uint8), D.some_inactive(rng, D.column_lens())):
                for cb, ce in RANGES:
                    a = D.scalar_gradients(cols, binary, y, dual, delta, active, cb, ce)
                    b = D.vector_gradients(*z, dic.size, y, dual, delta, active, cb, ce)
                    assert same(a[0], b[0]) and same(a[1], b[1])


@pytest.mark.parametrize("binary", (False, True))
def test_saturated_terms_are_exact(binary):
    """delta = 5 and dual within a factor 2 of 1: every term of U is .25 or
    .25 v v, so U checks the sum's order with no exp in the way."""
    z, y, dic, cols = build(binary)
    rng = np.random.default_rng(6)
    dual = np.exp2(rng.uniform(-1, 1, D.ROWS))
    _, U = D.scalar_gradients(cols, binary, y, dual, np.full(dic.size, 5.0),
                              np.ones(dic.size), 0, dic.size)
    for k, col in enumerate(cols):
        u = 0.0
        for _, v in col:
            u += .25 if binary else .25 * v * v
        assert D.bits(U[k:k + 1])[0] == D.bits(np.array([u]))[0]


@pytest.mark.parametrize("binary", (False, True))
@pytest.mark.parametrize("emax", (20, 1))
def test_forms_agree_on_update_dual(binary, emax):
    z, y, dic, cols = build(binary, emax)
    rng = np.random.default_rng(7)
    dual = D.spread_dual(rng, D.ROWS)
    cur_w = rng.standard_normal(dic.size)
    cur_w[::5] = 0.0
    delta = rng.uniform(0.1, 3.0, dic.size)
    active = D.some_inactive(rng, D.column_lens())
    for cb, ce in RANGES:
        nw = D.update_weights(rng, cur_w, cb, ce, DELTA_MAX) if ce - cb >= 7 else \
            cur_w[cb:ce] + 2.0 ** -10
        a = D.scalar_update_dual(cols, binary, y, dual, cur_w, delta, active, cb, ce, nw, DELTA_MAX)
        b = D.vector_update_dual(*z, dic.size, y, dual, cur_w, delta, active, cb, ce, nw,
                                 DELTA_MAX)
        for x, w in zip(a, b):
            assert same(x, np.asarray(w, x.dtype) if x.dtype != np.float64 else w)
        untouched = a[5] == 0
        assert untouched[0] and untouched[-1]
        assert same(a[0][untouched], dual[untouched])
        if ce - cb >= 7:
            assert np.any(a[1][cb:ce] != cur_w[cb:ce]) and np.any(a[2] == DELTA_MAX)
            assert np.sum(a[3]) < np.sum(active)


def test_forms_agree_on_init_and_objv():
    rng = np.random.default_rng(8)
    y = rng.choice([-1.0, 1.0], size=D.ROWS)
    xw = rng.standard_normal(D.ROWS) * 4
    assert same(D.scalar_init_dual(y, xw), D.vector_init_dual(y, xw))
    for dual in (D.special_dual(rng, D.ROWS), D.spread_dual(rng, D.ROWS), np.ones(D.ROWS)):
        a, b = D.scalar_objv(dual), D.vector_objv(dual)
        assert D.bits(np.array([a]))[0] == D.bits(np.array([b]))[0]
    assert D.scalar_objv(np.ones(4)) == 4 * np.log(2.0)


@pytest.mark.parametrize("rows", D.ROW_COUNTS)
def test_row_cases_tell_the_order_of_a_rows_factors(rows):
    """The cases of the sort by row (1, 2, 2 and 3 digit passes): the forms
    agree, the three full rows are where the docstring puts them, and
    multiplying a row's factors backwards changes the bits of some row."""
    offset, index, value, y, dic = D.row_case(rows)
    z = D.localized(offset, index, value, dic)
    passes = sum(1 for d in range(8) if ((1 << rows.bit_length()) - 1) >> (8 * d) & 0xFF)
    assert passes == {255: 1, 256: 2, 65535: 2, 65536: 3}[rows]
    lens = np.diff(offset.astype(np.int64))
    assert 100 <= index.size <= 400 and np.mean(lens == 0) > 0.7
    assert lens[0] == lens[rows // 2] == lens[-1] == 12 and np.sum(lens > 0) == 63
    dual, cur_w, delta, active, nw = D.row_case_update(rows)
    args = (dic.size, y, dual, cur_w, delta, active, 0, dic.size, nw, DELTA_MAX)
    a = D.scalar_update_dual(D.scalar_columns(*z, dic.size), False, y, *args[2:])
    b = D.vector_update_dual(*z, *args)
    for x, w in zip(a, b):
        assert same(x, np.asarray(w, x.dtype) if x.dtype != np.float64 else w)
    r = D.vector_update_dual(*z, *args, reverse=True)
    changed = D.bits(b[0]) != D.bits(r[0])
    print("rows %d: %d of %d rows with factors change when reversed"
          % (rows, changed.sum(), (b[5] > 0).sum()))
    assert changed.any() and np.isfinite(b[0]).all() and b[0].min() > 1e-300
    assert same(b[0][b[5] == 0], dual[b[5] == 0]) and (b[5] == 0).sum() >= rows - 63


REVERSED_SHARE = 0.30


def test_reversed_order_changes_G():
    """The valued case tells the reference's order from the reverse: G
    differs on at least REVERSED_SHARE of the columns of 8 entries or more
    (test_worker.py asks the same of its sums).  Measured on these 36 columns:
    G differs on 0.83 of them, U on 0.58."""
    z, y, dic, cols = build(False)
    rng = np.random.default_rng(9)
    dual = D.spread_dual(rng, D.ROWS)
    args = (cols, False, y, dual, np.ones(dic.size), np.ones(dic.size), 0, dic.size)
    G, U = D.scalar_gradients(*args)
    Gr, Ur = D.scalar_gradients(*args, reverse=True)
    long_ = D.column_lens() >= 8
    share_g = np.mean(D.bits(G)[long_] != D.bits(Gr)[long_])
    share_u = np.mean(D.bits(U)[long_] != D.bits(Ur)[long_])
    print("columns of >= 8 entries: %d, G differs on %.2f, U on %.2f"
          % (long_.sum(), share_g, share_u))
    assert long_.sum() >= 20
    assert share_g >= REVERSED_SHARE and share_u >= REVERSED_SHARE
