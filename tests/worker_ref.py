"""CPU restatements of the reference's online worker step, for the worker tests.

This is a RESTATEMENT.  Its localizer part (count_uniq, remap) is held to
the reference's compiled code: localizer.h is compiled in place into
oracle/_ref/libref_localizer.so, what it returns is recorded in
tests/golden/reference_pin/localizer.npz, and tests/test_reference_pin.py
holds both forms below to the recording bit for bit; only the order of
positions within a run of equal ids has no reference (std::sort leaves it
open; both forms are stable, as the product is).  The rest is unpinned
(DESIGN.md section 7): loss.h and base/matrix.h need Eigen, and countKeys
lives in ftrl.cc, which needs the whole solver.  There are two independent
forms that must agree bit for bit (tests/test_worker.py):

``scalar_*``  Python ints and floats (IEEE binary64, one correctly rounded
              operation per operator), loops in the reference's own order,
              ``math.exp`` / ``math.log``;
``vector_*``  numpy: ``np.unique(return_counts)``, ``searchsorted``, stable
              argsort for the transpose, and every ordered sum as
              ``np.add.accumulate`` (a sequential left fold) over the segment
              with the leading ``0`` of ``W y_i = 0`` in front.  exp and log
              are libm's here too (numpy's SIMD exp is not bit-identical to
              libm's); the arithmetic around them is numpy's.

Restated: Localizer::countUniqIndex (reference src/base/localizer.h:50-87),
Localizer::remapIndex (localizer.h:110-168), FTRL::countKeys
(src/linear_method/ftrl.cc:154-174), SparseMatrix::rangeTimes
(src/base/sparse_matrix.h:73-106, both branches; transTimes =
trans()->times, base/matrix.h:57-58), LogitLoss::evaluate / compute
(src/linear_method/loss.h:73-85).  Defined deviations of the product
(include/psg.h) are restated as the product defines them: an empty row has
Xw = +0.0, an empty dictionary is legal, objv is a serial sum here.
"""
import math

import numpy as np

U64 = np.uint64

# Mirrors of the kernels' constants, for the cases that are sized by them
# (tests/test_worker.py checks each against the line it copies): SORT_KPT,
# FLAG_TILE and row_scan_kernel are psg_sort.h's, the rest psg_worker.hip's.
# The sort tile is read from the library (psg_mb_sort_tile) and passed in.
SORT_KPT = 8      # PSG_SORT_KPT: the sort tile is 256 * SORT_KPT pairs
FLAG_TILE = 2048  # kFlagTile: elements per workgroup of the flag scans
LONG_RUN = 32     # PSG_LONG_RUN: a longer run is summed by a whole wave
LONG_GRID = 1024  # kLongGrid: workgroups of 4 waves over the long runs
CHAIN = 512       # 64 * PSG_CHAIN_AHEAD: terms per batch of chain_sum
CHAIN2 = 256      # 64 * PSG_CHAIN_AHEAD2: pairs of terms per batch of chain_sum2
SCAN = 256        # items per trip of row_scan_kernel and objv_kernel (a workgroup)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ scalar --
def scalar_count_uniq(index):
    """localizer.h:58-81: (sorted keys, sorted positions, uniq_key, key_cnt)."""
    idx = np.asarray(index, U64).tolist()
    pair = sorted(((k, i) for i, k in enumerate(idx)), key=lambda p: p[0])  # stable
    uniq, cnt = [], []
    if pair:
        curr, c = pair[0][0], 0
        for k, _ in pair:
            if k != curr:
                uniq.append(curr)
                curr = k
                cnt.append(c)
                c = 0
            c += 1
        uniq.append(curr)
        cnt.append(c)
    return (np.array([p[0] for p in pair], U64), np.array([p[1] for p in pair], np.uint32),
            np.array(uniq, U64), np.array(cnt, np.uint32))


def scalar_remap(offset, index, value, dic, skey, spos):
    """localizer.h:122-153: (new_offset, new_index, new_value, remapped)."""
    off = np.asarray(offset, U64).tolist()
    d = np.asarray(dic, U64).tolist()
    sk, sp = np.asarray(skey).tolist(), np.asarray(spos).tolist()
    val = None if value is None else np.asarray(value, np.float64).tolist()
    remapped = [0] * len(sk)
    cd = cp = 0
    while cd != len(d) and cp != len(sk):
        if d[cd] < sk[cp]:
            cd += 1
        else:
            if d[cd] == sk[cp]:
                remapped[sp[cp]] = cd + 1
            cp += 1
    new_index, new_value, new_offset = [], [], [0]
    for i in range(len(off) - 1):
        n = 0
        for j in range(off[i], off[i + 1]):
            if remapped[j] == 0:
                continue
            n += 1
            if val is not None:
                new_value.append(val[j])
            new_index.append(remapped[j] - 1)
        new_offset.append(new_offset[i] + n)
    return (np.array(new_offset, U64), np.array(new_index, np.uint32),
            np.array(new_value, np.float64), np.array(remapped, np.uint32))


def scalar_count_keys(y, new_offset, new_index, p):
    """ftrl.cc:164-173."""
    os_, idx, yy = np.asarray(new_offset).tolist(), np.asarray(new_index).tolist(), \
        np.asarray(y, np.float64).tolist()
    pos, neg = [0] * p, [0] * p
    for i in range(len(os_) - 1):
        tgt = pos if yy[i] > 0 else neg
        for j in range(os_[i], os_[i + 1]):
            tgt[idx[j]] += 1
    return np.array(pos, np.uint32), np.array(neg, np.uint32)


def scalar_times(new_offset, new_index, new_value, x, reverse=False):
    """sparse_matrix.h:75-86; an empty row is +0.0 (defined deviation).
    reverse: the same terms summed backwards (the order-sensitivity guard)."""
    os_, idx = np.asarray(new_offset).tolist(), np.asarray(new_index).tolist()
    xx = np.asarray(x, np.float64).tolist()
    binary = new_value is None or (len(new_value) == 0 and len(idx) > 0)
    val = None if binary else np.asarray(new_value, np.float64).tolist()
    out = []
    for i in range(len(os_) - 1):
        js = range(os_[i], os_[i + 1])
        y_i = 0.0
        for j in (reversed(js) if reverse else js):
            y_i += xx[idx[j]] if val is None else xx[idx[j]] * val[j]
        out.append(y_i)
    return np.array(out, np.float64)


def scalar_trans_times(new_offset, new_index, new_value, c, p, reverse=False):
    """sparse_matrix.h:88-104 on the transpose: rows in order, += into y[k]."""
    os_, idx = np.asarray(new_offset).tolist(), np.asarray(new_index).tolist()
    cc = np.asarray(c, np.float64).tolist()
    binary = new_value is None or (len(new_value) == 0 and len(idx) > 0)
    val = None if binary else np.asarray(new_value, np.float64).tolist()
    y = [0.0] * p
    rows = range(len(os_) - 1)
    for i in (reversed(rows) if reverse else rows):
        w_i = cc[i]
        js = range(os_[i], os_[i + 1])
        for j in (reversed(js) if reverse else js):
            y[idx[j]] += w_i if val is None else w_i * val[j]
    return np.array(y, np.float64)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def scalar_logit(y, xw):
    """loss.h:74,81: (tau, c = -y tau, loss, objv as the serial sum)."""
    tau, c, loss, objv = [], [], [], 0.0
    for yi, x in zip(np.asarray(y, np.float64).tolist(), np.asarray(xw, np.float64).tolist()):
        t = 1 / (1 + _exp(yi * x))
        s = 1 + _exp(-yi * x)
        l = math.log(s) if s != math.inf else math.inf
        tau.append(t)
        c.append(-yi * t)
        loss.append(l)
        objv += l
    return (np.array(tau, np.float64), np.array(c, np.float64), np.array(loss, np.float64), objv)


# ------------------------------------------------------------------ vector --
def vector_count_uniq(index):
    idx = np.asarray(index, U64)
    order = np.argsort(idx, kind="stable")
    uniq, cnt = np.unique(idx, return_counts=True)
    return idx[order], order.astype(np.uint32), uniq, cnt.astype(np.uint32)


def vector_remap(offset, index, value, dic, skey=None, spos=None):
    off, idx, d = np.asarray(offset, U64), np.asarray(index, U64), np.asarray(dic, U64)
    if d.size:
        r = np.minimum(np.searchsorted(d, idx), d.size - 1)
        hit = d[r] == idx
    else:
        r, hit = np.zeros(idx.size, np.int64), np.zeros(idx.size, bool)
    remapped = np.where(hit, r + 1, 0).astype(np.uint32)
    before = np.concatenate([[0], np.cumsum(hit)]).astype(U64)
    new_value = np.zeros(0, np.float64) if value is None else np.asarray(value, np.float64)[hit]
    return before[off.astype(np.int64)], (remapped[hit] - 1).astype(np.uint32), new_value, remapped


def vector_count_keys(y, new_offset, new_index, p):
    os_ = np.asarray(new_offset).astype(np.int64)
    row = np.repeat(np.arange(os_.size - 1), np.diff(os_))
    positive = (np.asarray(y, np.float64) > 0)[row]
    idx = np.asarray(new_index).astype(np.int64)
    return (np.bincount(idx[positive], minlength=p).astype(np.uint32),
            np.bincount(idx[~positive], minlength=p).astype(np.uint32))


def _fold(terms):
    """((0 + t0) + t1) + ... as np.add.accumulate computes it."""
    return np.add.accumulate(np.concatenate([[0.0], terms]))[-1]


def vector_times(new_offset, new_index, new_value, x):
    os_ = np.asarray(new_offset).astype(np.int64)
    idx = np.asarray(new_index).astype(np.int64)
    binary = new_value is None or (len(new_value) == 0 and idx.size > 0)
    terms = np.asarray(x, np.float64)[idx]
    if not binary:
        terms = terms * np.asarray(new_value, np.float64)
    return np.array([_fold(terms[os_[i]:os_[i + 1]]) for i in range(os_.size - 1)], np.float64)


def vector_trans_times(new_offset, new_index, new_value, c, p):
    os_ = np.asarray(new_offset).astype(np.int64)
    idx = np.asarray(new_index).astype(np.int64)
    binary = new_value is None or (len(new_value) == 0 and idx.size > 0)
    row = np.repeat(np.arange(os_.size - 1), np.diff(os_))
    terms = np.asarray(c, np.float64)[row]
    if not binary:
        terms = terms * np.asarray(new_value, np.float64)
    order = np.argsort(idx, kind="stable")  # the transpose: by column, then by position
    start = np.searchsorted(idx[order], np.arange(p + 1))
    t = terms[order]
    return np.array([_fold(t[start[k]:start[k + 1]]) for k in range(p)], np.float64)


_vexp = np.vectorize(_exp, otypes=[np.float64])
_vlog = np.vectorize(lambda s: math.log(s) if s != math.inf else math.inf, otypes=[np.float64])


def vector_logit(y, xw):
    y, xw = np.asarray(y, np.float64), np.asarray(xw, np.float64)
    if y.size == 0:
        z = np.zeros(0, np.float64)
        return z, z, z, 0.0
    with np.errstate(all="ignore"):
        tau = 1 / (1 + _vexp(y * xw))
        loss = _vlog(1 + _vexp(-y * xw))
    return tau, -y * tau, loss, float(_fold(loss))


# -------------------------------------------------------------- whole step --
class Step:
    """Everything one minibatch gives against dictionary `dic` and weights `w`."""

    def __init__(self, form, offset, index, value, y, dic, w=None):
        f = {"scalar": (scalar_count_uniq, scalar_remap, scalar_count_keys, scalar_times,
                        scalar_trans_times, scalar_logit),
             "vector": (vector_count_uniq, vector_remap, vector_count_keys, vector_times,
                        vector_trans_times, vector_logit)}[form]
        dic = np.asarray(dic, U64)
        self.skey, self.spos, self.uniq, self.cnt = f[0](index)
        self.new_offset, self.new_index, self.new_value, self.remapped = \
            f[1](offset, index, value, dic, self.skey, self.spos)
        self.nv = None if value is None else self.new_value
        self.pos, self.neg = f[2](y, self.new_offset, self.new_index, dic.size)
        if w is not None:
            self.xw = f[3](self.new_offset, self.new_index, self.nv, w)
            self.tau, self.c, self.loss, self.objv = f[5](y, self.xw)
            self.grad = f[4](self.new_offset, self.new_index, self.nv, self.c, dic.size)

    def arrays(self):
        return {k: v for k, v in vars(self).items() if isinstance(v, np.ndarray)}


def grad_bound(st, y):
    """Per column: (5 + n_k) 2^-52 sum |c v| over the column's n_k terms."""
    os_ = st.new_offset.astype(np.int64)
    row = np.repeat(np.arange(os_.size - 1), np.diff(os_))
    t = np.abs(st.c[row] * (st.nv if st.nv is not None else 1.0))
    idx = st.new_index.astype(np.int64)
    p = st.pos.size
    s = np.bincount(idx, weights=t, minlength=p)
    n = np.bincount(idx, minlength=p)
    return (5 + n) * 2.0 ** -52 * s


def loss_bound(loss):
    return 4 * 2.0 ** -52 * np.maximum(1.0, loss)


def objv_bound(loss):
    return loss.size * 2.0 ** -53 * float(np.sum(loss)) + float(np.sum(loss_bound(loss)))


def ulp_distance(a, b):
    """Distance in units of the last place between finite doubles of one sign."""
    ia = np.ascontiguousarray(a, np.float64).view(np.int64)
    ib = np.ascontiguousarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


# ---------------------------------------------------------- case generators --
def sensitive_values(rng, n):
    """N(0,1) 2^e, e uniform in -20..20: sums whose bits depend on the order."""
    return rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, size=n).astype(np.float64))


def special_vector(rng, n):
    """Random doubles with +0.0, -0.0 and a denormal among them."""
    v = sensitive_values(rng, n)
    if n >= 3:
        at = rng.choice(n, size=3, replace=False)
        v[at[0]], v[at[1]], v[at[2]] = 0.0, -0.0, 5e-324 * 12345
    return v


def csr_of(rng, index, rows, empty=()):
    """Splits `index` into `rows` rows at random cuts; rows in `empty` hold nothing."""
    n = len(index)
    live = [r for r in range(rows) if r not in set(empty)]
    cuts = np.sort(rng.integers(0, n + 1, size=max(len(live) - 1, 0)))
    lens = np.diff(np.concatenate([[0], cuts, [n]])) if live else np.zeros(0, np.int64)
    full = np.zeros(rows, np.int64)
    full[live] = lens
    return np.concatenate([[0], np.cumsum(full)]).astype(U64)


def sort_cases(tile):
    """name -> index array: every size and key pattern the sort must get right."""
    rng = np.random.default_rng(11)
    big = lambda n: rng.integers(0, 1 << 64, size=n, dtype=U64)  # noqa: E731
    c = {}
    sizes = {"n1": 1, "n63": 63, "n64": 64, "n65": 65, "tile_minus_1": tile - 1, "tile": tile,
             "tile_plus_1": tile + 1, "three_tiles_plus_7": 3 * tile + 7}
    for name, n in sizes.items():  # about three of each id, spread over all 64 bits
        c[name] = rng.integers(0, 50 + n // 3, size=n, dtype=U64) * U64(0x9E3779B97F4A7C15)
    c["one_key"] = np.full(2 * tile + 5, 0xDEADBEEF12345678, U64)
    c["distinct"] = rng.permutation(np.unique(big(tile + 300)))
    c["extremes"] = rng.permutation(np.concatenate(
        [big(500), np.zeros(3, U64), np.full(3, (1 << 64) - 1, U64)]))
    c["top_byte"] = rng.integers(0, 256, size=tile + 9, dtype=U64) << U64(56) | U64(0x1234567)
    c["bottom_byte"] = rng.integers(0, 256, size=tile + 9, dtype=U64) | U64(0xABCDEF0123456700)
    c["upper_six"] = rng.integers(0, 1 << 16, size=tile + 9, dtype=U64) | U64(0xABCDEF0123450000)
    # passes on digits that are not neighbours, and tile counts at which the
    # sort's tile permutation is no identity (9 or more, no multiple of 8)
    c["digits_0_3_7"] = digits_only(rng, tile + 9, (0, 3, 7))
    c["digits_1_2_4_5_6"] = digits_only(rng, tile + 9, (1, 2, 4, 5, 6))
    for name, n in (("nine_tiles_plus_5", 9 * tile + 5), ("seventeen_tiles_plus_3", 17 * tile + 3)):
        c[name] = rng.integers(0, 50 + n // 3, size=n, dtype=U64) * U64(0x9E3779B97F4A7C15)
    return c


def digits_only(rng, n, digits, fixed=0xA5C3E1967B2D4F08):
    """n keys whose bytes `digits` are random and whose other bytes are `fixed`'s."""
    mask = sum(0xFF << (8 * d) for d in digits)
    k = rng.integers(0, 1 << 64, size=n, dtype=U64) & U64(mask)
    return k | U64(fixed & ~mask & ((1 << 64) - 1))


def zipf_ids(rng, n, universe=5000, a=1.1):
    p = np.arange(1, universe + 1, dtype=np.float64) ** -a
    table = np.unique(rng.integers(0, 1 << 64, size=universe + 64, dtype=U64))[:universe]
    table = rng.permutation(table)
    return table[rng.choice(universe, size=n, p=p / p.sum())]


def labels(rng, n, kinds=(1.0, -1.0)):
    return np.asarray(kinds, np.float64)[rng.integers(0, len(kinds), size=n)]


ODD_LABELS = (1.0, -1.0, 0.0, -0.0, 2.5, float("nan"))


def zipf_case(seed=3, rows=300, mean=12, binary=False, kinds=(1.0, -1.0)):
    """300 rows x ~12 Zipf ids: the head key's run is some hundreds long, most
    runs are 1-3; rows 0, 7, 8 and the last are empty; row 1 holds one id twice
    with different values."""
    rng = np.random.default_rng(seed)
    index = zipf_ids(rng, rows * mean)
    offset = csr_of(rng, index, rows, empty=(0, 7, 8, rows - 1))
    a = int(offset[1])
    assert int(offset[2]) - a >= 2
    index[a + 1] = index[a]
    value = None if binary else sensitive_values(rng, index.size)
    return offset, index, value, labels(rng, rows, kinds)


def column_case(seed=5, rows=2000):
    """Every row holds key K (so its run is `rows` long) and two Zipf ids."""
    rng = np.random.default_rng(seed)
    index = zipf_ids(rng, 3 * rows).reshape(rows, 3)
    index[:, 1] = U64(0x7777777777777777)
    index = index.reshape(-1)
    offset = (np.arange(rows + 1) * 3).astype(U64)
    return offset, index, sensitive_values(rng, index.size), labels(rng, rows)


def absent_keys(rng, uniq, n):
    """n keys not in uniq, one below its minimum and one above its maximum
    (uniq must leave room at both ends)."""
    lo, hi = int(uniq.min()), int(uniq.max())
    assert lo > 0 and hi < (1 << 64) - 1
    c = np.unique(rng.integers(lo, hi, size=2 * n + 16, dtype=U64))
    c = rng.permutation(c[~np.isin(c, uniq)])[:n - 2]
    return np.concatenate([c, np.array([lo - 1, hi + 1], U64)])


def dict_cases(uniq, seed=17):
    """name -> dictionary (strictly increasing) for a minibatch whose keys are uniq."""
    rng = np.random.default_rng(seed)
    return {
        "all": uniq.copy(),
        "every_other": uniq[::2].copy(),
        "with_absent": np.unique(np.concatenate([uniq, absent_keys(rng, uniq, 50)])),
        "empty": np.zeros(0, U64),
        "single": uniq[uniq.size // 2:uniq.size // 2 + 1].copy(),
    }


def branch_report(offset, index, value, dic):
    """Which of the localiser's branches a (minibatch, dictionary) pair takes."""
    off = np.asarray(offset).astype(np.int64)
    lens = np.diff(off)
    kept = np.isin(index, dic)
    kept_per_row = np.add.reduceat(np.concatenate([kept, [False]]).astype(np.int64),
                                   np.minimum(off[:-1], kept.size))
    kept_per_row[lens == 0] = 0
    twice = False
    for i in np.nonzero(lens >= 2)[0]:
        row = index[off[i]:off[i + 1]]
        u, cnt = np.unique(row, return_counts=True)
        for k in u[cnt >= 2]:
            at = np.nonzero(row == k)[0]
            if kept[off[i] + at[0]] and (value is None or
                                         value[off[i] + at[0]] != value[off[i] + at[1]]):
                twice = True
    uniq = np.unique(index)
    return {
        "empty_first": bool(lens[0] == 0), "empty_last": bool(lens[-1] == 0),
        "empty_consecutive": bool(np.any((lens[:-1] == 0) & (lens[1:] == 0))),
        "emptied_by_dict": bool(np.any((lens > 0) & (kept_per_row == 0))),
        "id_twice_in_row": twice,
        "dropped": bool(np.any(~kept)), "kept": bool(np.any(kept)),
        "dict_below_min": bool(dic.size and uniq.size and dic[0] < uniq[0]),
        "dict_above_max": bool(dic.size and uniq.size and dic[-1] > uniq[-1]),
        "dict_absent_inside": bool(np.any(~np.isin(dic, uniq))),
        "run_over_wave": bool(uniq.size and np.unique(index, return_counts=True)[1].max() > 64),
    }


# ------------------------------------------------------------ the seam case --
# One minibatch past the first iteration of every second-level structure of
# psg_worker.hip: more than SCAN tiles in the sort and in both flag scans (so
# row_scan_kernel carries), tile counts that are no multiple of 8 (xcd_index is
# a real permutation), more long runs than the 4 * LONG_GRID waves of the
# long-run kernels, more than SCAN partial sums of the objective, and a run at
# each edge of the short / long split and of a chain_sum batch.
SEAM_EDGE_RUNS = (LONG_RUN, LONG_RUN + 1, 64, 65, CHAIN - 1, CHAIN, CHAIN + 1, 2 * CHAIN,
                  2 * CHAIN + 1)


def seam_case(tile, seed, binary=False, n=None, rows=None, long_keys=None, values=None):
    """(offset, index, value, y).  n pairs (default 257 max(tile, FLAG_TILE) +
    1) in `rows` rows (default 256 SCAN + 301; rows 0, 7, 8 and the last are
    empty): one key for each run length of SEAM_EDGE_RUNS, `long_keys` keys
    (default 4 LONG_GRID + 100) with runs of 33 .. 47, and keys with runs of
    1 .. 8 for the rest; the keys are spread over all 64 bits and the pairs
    shuffled.  values(rng, n) gives the values (default sensitive_values).
    n, rows and long_keys are there for a cut-down case the scalar form can
    finish; such a case makes no claim about tile counts."""
    rng = np.random.default_rng(seed)
    n = (SCAN + 1) * max(tile, FLAG_TILE) + 1 if n is None else n
    rows = SCAN * 256 + 301 if rows is None else rows
    long_keys = 4 * LONG_GRID + 100 if long_keys is None else long_keys
    lens = np.concatenate([np.array(SEAM_EDGE_RUNS, np.int64),
                           rng.integers(LONG_RUN + 1, LONG_RUN + 16, size=long_keys)])
    rest = n - int(lens.sum())
    assert rest > 0, "no room for the short runs"
    short = rng.integers(1, 9, size=rest)
    short = short[:int(np.searchsorted(np.cumsum(short), rest)) + 1]
    short[-1] -= int(short.sum()) - rest
    lens = rng.permutation(np.concatenate([lens, short[short > 0]]))  # key order is not length order
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=lens.size + 64, dtype=U64))
    assert keys.size >= lens.size
    keys = rng.permutation(keys)[:lens.size]
    index = rng.permutation(np.repeat(keys, lens))
    assert index.size == n
    offset = csr_of(rng, index, rows, empty=(0, 7, 8, rows - 1))
    value = None if binary else (sensitive_values if values is None else values)(rng, n)
    return offset, index, value, labels(rng, rows)


def seam_dict(index, seed=17, every=97):
    """dict_cases' "with_absent" without about every 97th data key (the keys of
    the edge-length runs stay): pairs are kept and dropped all over the
    minibatch, and dictionary keys have no run."""
    uniq, cnt = np.unique(index, return_counts=True)
    dic = dict_cases(uniq, seed)["with_absent"]
    gone = np.zeros(uniq.size, bool)
    gone[::every] = True
    gone &= ~np.isin(cnt, SEAM_EDGE_RUNS[:1] + SEAM_EDGE_RUNS[2:])  # 33 is a common length
    first33 = np.nonzero(cnt == SEAM_EDGE_RUNS[1])[0][:1]
    gone[first33] = False
    return dic[~np.isin(dic, uniq[gone])]


def seam_report(offset, index, dic, tile):
    """What of the device code's second-level structure a (minibatch,
    dictionary) pair reaches; tests/test_worker.py asserts on it."""
    off = np.asarray(offset).astype(np.int64)
    n, rows = index.size, off.size - 1
    uniq, cnt = np.unique(index, return_counts=True)
    dic_cnt = cnt[np.isin(uniq, dic)]
    differ = int(np.bitwise_or.reduce(index) ^ np.bitwise_and.reduce(index))
    passes = [d for d in range(8) if (differ >> (8 * d)) & 0xFF]
    # the order in which pass d reads the pairs: stably sorted on the digits below d
    carry_passes, edge = [], SCAN * tile
    for d in passes:
        order = np.argsort(index & U64((1 << (8 * d)) - 1), kind="stable")
        digit = ((index[order] >> U64(8 * d)) & U64(0xFF)).astype(np.int64)
        if np.intersect1d(digit[:edge], digit[edge:]).size:  # the digit's scan adds a carry
            carry_passes.append(d)
    skey = np.sort(index)
    head = np.concatenate([[True], skey[1:] != skey[:-1]])
    kept = np.isin(index, dic)
    fedge = SCAN * FLAG_TILE
    lens = np.diff(off)
    return {
        "pairs": n, "rows": rows, "keys": int(uniq.size), "dict": int(dic.size),
        "sort_tiles": -(-n // tile), "flag_tiles": -(-n // FLAG_TILE),
        "long_dict_keys": int(np.sum(dic_cnt > LONG_RUN)),
        "dict_run_lengths": set(dic_cnt.tolist()),
        "loss_partials": -(-rows // SCAN),
        "differing_digits": len(passes), "carry_passes": carry_passes,
        "heads_before": int(head[:fedge].sum()), "heads_after": int(head[fedge:].sum()),
        "kept_before": int(kept[:fedge].sum()), "kept_after": int(kept[fedge:].sum()),
        "dropped_before": int((~kept[:fedge]).sum()), "dropped_after": int((~kept[fedge:]).sum()),
        "dict_absent": int(np.sum(~np.isin(dic, uniq))),
        "long_dropped": int(np.sum(cnt[~np.isin(uniq, dic)] > LONG_RUN)),
        "empty_rows": [int(r) for r in np.nonzero(lens == 0)[0][:3]] + [int(lens[-1] == 0)],
    }


RUN_EDGES = (1, LONG_RUN - 1, LONG_RUN, LONG_RUN + 1, 63, 64, 65, CHAIN - 1, CHAIN, CHAIN + 1,
             2 * CHAIN - 1, 2 * CHAIN, 2 * CHAIN + 1)


def run_edge_case(seed=31, rows=600, binary=False):
    """(offset, index, value, y, dic): one key for each run length of
    RUN_EDGES, key order not length order, and two dictionary keys (one inside,
    one above) that the data lacks."""
    rng = np.random.default_rng(seed)
    lens = rng.permutation(np.array(RUN_EDGES, np.int64))
    keys = np.unique(rng.integers(1, (1 << 64) - 1, size=lens.size + 1, dtype=U64))
    assert keys.size == lens.size + 1
    inside = keys[lens.size // 2]
    keys = np.delete(keys, lens.size // 2)
    index = rng.permutation(np.repeat(keys, lens))
    offset = csr_of(rng, index, rows, empty=(0, rows - 1))
    value = None if binary else sensitive_values(rng, index.size)
    dic = np.unique(np.concatenate([keys, [inside, keys.max() + U64(1)]]).astype(U64))
    return offset, index, value, labels(rng, rows), dic


def closed_loop_batches(seed=23, nbatch=5, rows=200, mean=10, universe=800):
    """Minibatches of Zipf ids over one table of ids, so their keys overlap."""
    table = np.unique(np.random.default_rng(seed).integers(
        1, (1 << 64) - 1, size=universe + 100, dtype=U64))[:universe]
    p = np.arange(1, universe + 1, dtype=np.float64) ** -1.05
    out = []
    for b in range(nbatch):
        rng = np.random.default_rng(seed * 100 + b)
        index = table[rng.choice(universe, size=rows * mean, p=p / p.sum())]
        offset = csr_of(rng, index, rows)
        out.append((offset, index, 0.25 * rng.standard_normal(index.size), labels(rng, rows)))
    return out
