"""CPU restatements of the worker half of the batch solver, for its tests.

This is a RESTATEMENT, not the reference's compiled code: darling.cc cannot
be compiled in place (it needs protobuf, glog, gflags and Eigen, none of which
is in the image), so parity with the reference is unpinned here (DESIGN.md
section 7).  To make up for it there are two independent forms that must agree
bit for bit (tests/test_darling_worker.py):

``scalar_*``  Python floats (IEEE binary64, one correctly rounded operation
              per operator), the loops of darling.cc:328-355 and :364-434 line
              by line over a column-major matrix filled as
              SparseMatrix::alterStorage fills it (sparse_matrix.h:186-241:
              each column in row-major scan order), ``math.exp``;
``vector_*``  numpy, sharing no code with the scalar form: stable argsort for
              the columns, and for the rows' factor lists, every ordered sum
              as ``np.add.accumulate`` and every ordered product as
              ``np.multiply.accumulate`` (sequential left folds) with the
              starting value in front.  exp is libm's here too (numpy's SIMD
              exp is not bit-identical to libm's).

Restated: Darling::computeGradients (reference
src/linear_method/darling.cc:306-356), updateDual (:358-435) with newDelta and
inactive (darling.h:31-35), the worker's line of preprocessData (:110) and of
evaluateProgress (:506, as a serial sum).  ``std::min(a, b)`` is ``b if b < a
else a``: a NaN first argument stays a NaN.
"""
import math

import numpy as np

INACTIVE = np.array([0xFFFFFFFFFFFFFFFF], np.uint64).view(np.float64)[0]  # kInactiveValue_


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _std_min(a, b):
    return b if b < a else a


# ------------------------------------------------------------------ scalar --
def scalar_columns(new_offset, new_index, new_value, p):
    """alterStorage: column k's (row, value) pairs in row-major scan order."""
    os_, idx = np.asarray(new_offset).tolist(), np.asarray(new_index).tolist()
    val = None if new_value is None else np.asarray(new_value, np.float64).tolist()
    cols = [[] for _ in range(p)]
    for i in range(len(os_) - 1):
        for j in range(os_[i], os_[i + 1]):
            cols[idx[j]].append((i, None if val is None else val[j]))
    return cols


def scalar_init_dual(y, xw):
    """darling.cc:110."""
    return np.array([_exp(a * b) for a, b in zip(np.asarray(y, np.float64).tolist(),
                                                 np.asarray(xw, np.float64).tolist())],
                    np.float64)


def scalar_gradients(cols, binary, y, dual, delta, active, cb, ce, reverse=False):
    """darling.cc:328-355 over columns [cb, ce): (G, U).  reverse: each
    column's entries backwards (the order-sensitivity guard)."""
    y, dual = np.asarray(y, np.float64).tolist(), np.asarray(dual, np.float64).tolist()
    delta, active = np.asarray(delta, np.float64).tolist(), np.asarray(active).tolist()
    G, U = [], []
    for k in range(cb, ce):
        if not active[k]:
            G.append(INACTIVE)
            U.append(INACTIVE)
            continue
        g, u = 0.0, 0.0
        d = _exp(delta[k]) if binary else delta[k]
        for i, v in (reversed(cols[k]) if reverse else cols[k]):
            tau = 1 / (1 + dual[i])
            if binary:
                g -= y[i] * tau
                u += _std_min(tau * (1 - tau) * d, .25)
            else:
                g -= y[i] * tau * v
                u += _std_min(tau * (1 - tau) * _exp(math.fabs(v) * d), .25) * v * v
        G.append(g)
        U.append(u)
    return np.array(G, np.float64), np.array(U, np.float64)


def scalar_update_dual(cols, binary, y, dual, cur_w, delta, active, cb, ce, new_w, delta_max):
    """darling.cc:364-378 and :420-434: (dual, cur_w, delta, active, delta_w)
    on copies; the factor count of every row as a sixth item."""
    y = np.asarray(y, np.float64).tolist()
    dual, cur_w = np.array(dual, np.float64).tolist(), np.array(cur_w, np.float64).tolist()
    delta, active = np.array(delta, np.float64).tolist(), np.array(active, np.uint8).tolist()
    new_w = np.asarray(new_w, np.float64).tolist()
    delta_w = [0.0] * len(new_w)
    for i in range(len(new_w)):
        j = cb + i
        nw = new_w[i]
        if nw != nw:
            active[j] = 0
            cur_w[j] = 0.0
            delta_w[i] = 0.0
            continue
        delta_w[i] = nw - cur_w[j]
        delta[j] = _std_min(delta_max, 2 * math.fabs(delta_w[i]) + .1)
        cur_w[j] = nw
    nfac = [0] * len(dual)
    for j in range(ce - cb):
        k = j + cb
        wd = delta_w[j]
        if wd == 0 or not active[k]:
            continue
        for i, v in cols[k]:
            dual[i] *= _exp(y[i] * wd) if binary else _exp(y[i] * wd * v)
            nfac[i] += 1
    return (np.array(dual, np.float64), np.array(cur_w, np.float64), np.array(delta, np.float64),
            np.array(active, np.uint8), np.array(delta_w, np.float64), np.array(nfac, np.int64))


def _log_term(d):
    r = math.copysign(math.inf, d) if d == 0 else 1 / d
    s = 1 + r
    return math.log(s) if s != math.inf else math.inf


def scalar_objv_terms(dual):
    return np.array([_log_term(d) for d in np.asarray(dual, np.float64).tolist()], np.float64)


def scalar_objv(dual):
    """darling.cc:506 as a serial sum."""
    o = 0.0
    for l in scalar_objv_terms(dual).tolist():
        o += l
    return o


# ------------------------------------------------------------------ vector --
_vexp = np.vectorize(_exp, otypes=[np.float64])


def _csc(new_offset, new_index, new_value, p):
    os_ = np.asarray(new_offset).astype(np.int64)
    idx = np.asarray(new_index).astype(np.int64)
    row = np.repeat(np.arange(os_.size - 1), np.diff(os_))
    order = np.argsort(idx, kind="stable")  # by column, then by position
    start = np.searchsorted(idx[order], np.arange(p + 1))
    val = None if new_value is None else np.asarray(new_value, np.float64)[order]
    return row[order], val, start, idx[order]


def vector_init_dual(y, xw):
    with np.errstate(all="ignore"):
        return _vexp(np.asarray(y, np.float64) * np.asarray(xw, np.float64))


def vector_gradients(new_offset, new_index, new_value, p, y, dual, delta, active, cb, ce):
    row, val, start, _ = _csc(new_offset, new_index, new_value, p)
    y, dual = np.asarray(y, np.float64), np.asarray(dual, np.float64)
    delta, active = np.asarray(delta, np.float64), np.asarray(active).astype(bool)
    with np.errstate(all="ignore"):
        tau = 1 / (1 + dual[row])
        q = tau * (1 - tau)
        if val is None:
            tg = y[row] * tau
            a = q * np.repeat(_vexp(delta), np.diff(start))
            tu = np.where(.25 < a, .25, a)
        else:
            tg = y[row] * tau * val
            a = q * _vexp(np.fabs(val) * np.repeat(delta, np.diff(start)))
            tu = np.where(.25 < a, .25, a) * val * val
    G, U = np.empty(ce - cb), np.empty(ce - cb)
    for k in range(cb, ce):
        if not active[k]:
            G[k - cb] = U[k - cb] = INACTIVE
            continue
        s = slice(start[k], start[k + 1])
        G[k - cb] = np.subtract.accumulate(np.concatenate([[0.0], tg[s]]))[-1]
        U[k - cb] = np.add.accumulate(np.concatenate([[0.0], tu[s]]))[-1]
    return G, U


def vector_update_dual(new_offset, new_index, new_value, p, y, dual, cur_w, delta, active, cb, ce,
                       new_w, delta_max, reverse=False):
    """reverse: each row's factors backwards (the order-sensitivity guard)."""
    row, val, start, col = _csc(new_offset, new_index, new_value, p)
    y, dual = np.asarray(y, np.float64), np.array(dual, np.float64)
    cur_w, delta = np.array(cur_w, np.float64), np.array(delta, np.float64)
    active, new_w = np.array(active, np.uint8), np.asarray(new_w, np.float64)
    blk = slice(cb, ce)
    nan = np.isnan(new_w)
    with np.errstate(all="ignore"):
        delta_w = np.where(nan, 0.0, new_w - cur_w[blk])
        nd = 2 * np.fabs(delta_w) + .1
    delta[blk] = np.where(nan, delta[blk], np.where(nd < delta_max, nd, delta_max))
    cur_w[blk] = np.where(nan, 0.0, new_w)
    active[blk] = np.where(nan, 0, active[blk])
    wd_all = np.zeros(p)
    wd_all[blk] = delta_w
    live = (wd_all != 0) & active.astype(bool)
    live[:cb] = False
    live[ce:] = False
    keep = live[col]  # entries in (column, position) order whose column contributes
    r, wd = row[keep], wd_all[col[keep]]
    with np.errstate(all="ignore"):
        f = _vexp(y[r] * wd) if val is None else _vexp(y[r] * wd * val[keep])
    by_row = np.argsort(r, kind="stable")  # a row's factors stay in (column, position) order
    rs = np.searchsorted(r[by_row], np.arange(dual.size + 1))
    f = f[by_row]
    with np.errstate(all="ignore"):
        for i in np.nonzero(np.diff(rs))[0]:
            fi = f[rs[i]:rs[i + 1]][::-1] if reverse else f[rs[i]:rs[i + 1]]
            dual[i] = np.multiply.accumulate(np.concatenate([[dual[i]], fi]))[-1]
    return dual, cur_w, delta, active, delta_w, np.diff(rs)


def vector_objv(dual):
    with np.errstate(all="ignore"):
        s = 1 + 1 / np.asarray(dual, np.float64)
    t = np.array([math.log(x) if x != math.inf else math.inf for x in s.tolist()], np.float64)
    return float(np.add.accumulate(np.concatenate([[0.0], t]))[-1])


# ------------------------------------------------------------------ bounds --
# Both sides run the same operations on the same inputs, and differ in exp /
# log alone: each side's is within 1 ulp of the true value (the device's by the
# premise of include/psg.h, libm's by its documentation), so two results are
# within 2 x 2^-52 of each other, relatively.  Every rounded operation after
# that adds 2^-53 per side, 2^-52 for the pair.  Bounds are first order in
# 2^-52; one more unit of 2^-52 in each constant pays for every higher-order
# term at these sizes (n < 2^20).
def u_bound(U, n_k, binary):
    """Per column of n_k terms.  A term: exp 2, the product with tau (1 - tau)
    1 (min moves two values no further apart), the valued form's two
    products with v 2 more; the argument of exp is the same on both sides.
    The terms are not negative, so the two chains of n_k adds are each within
    n_k 2^-53 U of the exact sum of their own terms: (c + n_k) 2^-52 U with
    c = 3 + 1 (binary) or 5 + 1 (valued)."""
    return ((4 if binary else 6) + np.asarray(n_k)) * 2.0 ** -52 * np.abs(U)


def dual_bound(dual, n_i):
    """Per row of n_i factors: exp 2 and the multiply 1 for each factor,
    c n_i 2^-52 dual with c = 3 + 1."""
    return 4 * np.asarray(n_i) * 2.0 ** -52 * np.abs(dual)


def init_bound(dual):
    """y * Xw is the same on both sides: the bound for one exp."""
    return 2 * 2.0 ** -52 * np.abs(dual)


def objv_bound(terms):
    """The device's fixed-order reduction is within rows 2^-53 objv of the
    exact sum of its terms (include/psg.h); a term's 1 / dual and 1 + are the
    same on both sides, its log is within 2 x 2^-52 of the host's.  Against
    math.fsum of the host's terms, which is the exact sum rounded once."""
    t = np.asarray(terms, np.float64)
    return (t.size + 1) * 2.0 ** -53 * float(np.sum(t)) + float(np.sum(2 * 2.0 ** -52 * t))


# ---------------------------------------------------------- case generators --
ROWS = 300
# the length of every dictionary column, by dictionary position: every path of
# the ordered sums (kLongRun = 32, one chain_sum batch = 512 terms), long
# columns on both sides of the inner range [4, 11), three keys absent from
# the data (0, 7 and the last)
HEAD_LENS = (0, 1, 32, 700, 5, 33, 64, 0, 200, 512, 3, 513)
INNER = (4, 11)


def column_lens(seed=1):
    rng = np.random.default_rng(seed)
    tail = rng.integers(1, 21, size=48)
    tail[18] = 40
    tail[-1] = 0
    return np.concatenate([HEAD_LENS, tail]).astype(np.int64)


def case(binary, emax=20, seed=1):
    """(offset, index, value, y, dic): ROWS rows, rows 0 and ROWS - 1 empty,
    60 dictionary keys with column_lens() entries each (a column longer than
    the row count repeats inside rows, sometimes side by side), and two data
    ids the dictionary lacks, one of them below its smallest key.  Values are
    +-[0.5, 1.5) 2^e, e in -4 .. emax: sums whose bits depend on the order,
    and |v| >= 2^-5."""
    rng = np.random.default_rng(seed)
    lens = column_lens(seed)
    dic = np.sort(rng.choice(np.arange(1, 1 << 20, dtype=np.uint64), size=lens.size,
                             replace=False)) * np.uint64(0x000003FFFF000001) + np.uint64(1 << 40)
    extra = np.array([int(dic[0]) - 5, int(dic[20]) + 1], np.uint64)
    live = np.arange(1, ROWS - 1)
    per_row = [[] for _ in range(ROWS)]
    for key, n in list(zip(dic.tolist(), lens.tolist())) + [(int(extra[0]), 7), (int(extra[1]), 9)]:
        whole, rest = divmod(n, live.size)
        rows = np.concatenate([np.repeat(live, whole), rng.choice(live, size=rest, replace=False)])
        for r in rows.tolist():
            per_row[r].append(key)
    index = []
    for r in range(ROWS):
        ids = np.array(per_row[r], np.uint64)
        index.append(ids[rng.permutation(ids.size)] if r % 2 else np.sort(ids))
    offset = np.concatenate([[0], np.cumsum([a.size for a in index])]).astype(np.uint64)
    index = np.concatenate(index).astype(np.uint64)
    value = None if binary else values(rng, index.size, emax)
    y = rng.choice([-1.0, 1.0], size=ROWS)
    return offset, index, value, y, dic


def values(rng, n, emax):
    """+-[0.5, 1.5) 2^e, e in -4 .. emax."""
    return (rng.choice([-1.0, 1.0], size=n) * (0.5 + rng.random(n))
            * np.exp2(rng.integers(-4, emax + 1, size=n).astype(np.float64)))


SEAM_SEED, SEAM_EMAX = 29, 2


def seam_case(tile):
    """(offset, index, value, y, dic): worker_ref.seam_case's structure (its
    docstring says what it reaches) with this module's values, e in -4 ..
    SEAM_EMAX so that G and U stay finite, against worker_ref.seam_dict."""
    import worker_ref as R
    offset, index, value, y = R.seam_case(
        tile, SEAM_SEED, values=lambda rng, n: values(rng, n, SEAM_EMAX))
    return offset, index, value, y, R.seam_dict(index)


ROW_COUNTS = (255, 256, 65535, 65536)  # 1, 2, 2 and 3 digit passes of the sort by row


def row_case(rows, seed=37):
    """(offset, index, value, y, dic): some hundred pairs over 40 keys in
    `rows` rows, most of them empty; the first row, the last and one in the
    middle hold 12 factors each, 60 others 1 .. 5."""
    rng = np.random.default_rng(seed + rows)
    dic = np.sort(rng.choice(np.arange(1, 1 << 20, dtype=np.uint64), size=40, replace=False)
                  ) * np.uint64(0x000003FFFF000001) + np.uint64(1 << 40)
    lens = np.zeros(rows, np.int64)
    lens[rng.choice(np.arange(1, rows - 1), size=60, replace=False)] = rng.integers(1, 6, size=60)
    lens[[0, rows // 2, rows - 1]] = 12
    index = dic[rng.integers(0, dic.size, size=int(lens.sum()))]
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return offset, index, values(rng, index.size, 1), rng.choice([-1.0, 1.0], size=rows), dic


def row_case_update(rows):
    """(dual, cur_w, delta, active, new_w) for one update_dual over all the
    columns of row_case(rows): steps of some tenths, so that the factors'
    mantissas are arbitrary and their order shows in the product."""
    rng = np.random.default_rng(1000 + rows)
    cur_w = rng.standard_normal(40)
    return (spread_dual(rng, rows), cur_w, rng.uniform(0.1, 3.0, 40), np.ones(40, np.uint8),
            cur_w + rng.standard_normal(40) * 0.3)


def localized(offset, index, value, dic):
    """Z of the case: (new_offset, new_index, new_value or None)."""
    hit = np.isin(index, dic)
    before = np.concatenate([[0], np.cumsum(hit)])
    new_index = np.searchsorted(dic, index[hit]).astype(np.uint32)
    return (before[offset.astype(np.int64)].astype(np.uint64), new_index,
            None if value is None else value[hit])


def special_dual(rng, n):
    """e^N(0, 15/3) with 0, +inf, two denormals and 1.0 among them."""
    d = np.exp(np.clip(rng.standard_normal(n) * 5, -15, 15))
    at = rng.choice(np.arange(1, n - 1), size=5, replace=False)
    d[at] = [0.0, np.inf, 5e-324, 5e-324 * 98765, 1.0]
    return d


def spread_dual(rng, n):
    """e^u, u uniform in -15 .. 15."""
    return np.exp(rng.uniform(-15, 15, size=n))


def some_inactive(rng, lens):
    """Active bytes with an inactive column of every kind of length."""
    a = np.ones(lens.size, np.uint8)
    a[[1, 6, 7, 11, 13, 14]] = 0  # lengths 1, 64, 0, 513 and two of the tail
    return a


def update_weights(rng, cur_w, cb, ce, delta_max):
    """new_w for columns [cb, ce): mostly cur_w + small steps, and by
    position in the block: the all-ones NaN, another NaN, +0.0, -0.0, cur_w
    itself, and two steps large enough for newDelta to return delta_max."""
    m = ce - cb
    assert m >= 7
    nw = cur_w[cb:ce] + rng.standard_normal(m) * 2.0 ** -18
    sp = [INACTIVE, np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0], 0.0, -0.0,
          None, None, None]
    at = rng.permutation(m)[:len(sp)]
    for a, s in zip(at.tolist(), sp):
        nw[a] = cur_w[cb + a] if s is None else s
    nw[at[5]] += delta_max
    nw[at[6]] -= 2 * delta_max
    return nw
