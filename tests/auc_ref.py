"""CPU restatements of the reference's evaluation, for the AUC tests.

This is a RESTATEMENT, held to the reference's compiled code: auc.h and
evaluation.h are compiled in place into oracle/_ref/libref_auc.so, what they
return is recorded in tests/golden/reference_pin/{auc,auc_merge,exact_auc}.npz,
and tests/test_reference_pin.py holds both forms below to those recordings
bit for bit.  What has no reference stays unpinned, on
the two forms' agreement alone (tests/test_auc.py): evaluate by key, and the
exact AUC where predictions tie across the two classes.  As in worker_ref.py
there are two independent forms that must agree bit for bit:

``scalar_*``  dicts, Python ints and floats (IEEE binary64, one correctly
              rounded operation per operator), the reference's own loops;
``vector_*``  numpy: ``np.unique``, a stable argsort, ``searchsorted`` and
              every ordered double sum as ``np.add.accumulate`` (a sequential
              left fold).

Restated: AUC::compute (reference src/base/auc.h:69-98), AUC::merge
(:14-22), AUC::accuracy (:26-39), AUC::evaluate (:42-59) as written and with
the loop condition of :49 read by key, and Evaluation<double>::auc
(src/base/evaluation.h:17-44) with a stable sort.  Defined deviations of the
product (include/psg.h) are restated as the product defines them: a NaN or
out-of-range product gets the key INT64_MIN, merge drops zero counts, 0 / 0
is NaN.

An AUCData is a tuple (tp_key int64, tp_count uint64, fp_key, fp_count), each
list ascending by key.
"""
import math

import numpy as np

INT64_MIN = -(1 << 63)
I64, U64, F64 = np.int64, np.uint64, np.float64


def bits(v):
    return np.ascontiguousarray(v, F64).view(U64)


def _data(tp, fp):
    tk, fk = sorted(tp), sorted(fp)
    return (np.array(tk, I64), np.array([tp[k] for k in tk], U64),
            np.array(fk, I64), np.array([fp[k] for k in fk], U64))


def same_data(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
               for x, y in zip(a, b)) and len(a) == len(b) == 4


# ------------------------------------------------------------------ scalar --
def scalar_key(p, goodness):
    prod = float(p) * float(goodness)  # auc.h:75: one rounded multiply
    if prod != prod or abs(prod) >= 2.0 ** 63:
        return INT64_MIN  # cvttsd2si's answer for what C++ leaves undefined
    return int(prod)  # truncation toward zero


def scalar_compute(y, predict, goodness):
    tp, fp = {}, {}
    for yi, pi in zip(np.asarray(y, F64).tolist(), np.asarray(predict, F64).tolist()):
        k = scalar_key(pi, goodness)
        side = tp if yi > 0 else fp  # auc.h:76; a NaN label is not > 0
        side[k] = side.get(k, 0) + 1
    return _data(tp, fp)


def scalar_merge(datas):
    """merge of several AUCData, whose lists may be unsorted and repeat keys."""
    tp, fp = {}, {}
    for tk, tc, fk, fc in datas:
        for side, keys, counts in ((tp, tk, tc), (fp, fk, fc)):
            for k, c in zip(np.asarray(keys).tolist(), np.asarray(counts).tolist()):
                if c:
                    side[k] = side.get(k, 0) + c
    return _data(tp, fp)


def scalar_accuracy(data, goodness, threshold=0.0):
    tk, tc, fk, fc = [np.asarray(a).tolist() for a in data]
    total = correct = 0.0
    x = float(threshold) * float(goodness)
    for k, c in zip(tk, tc):
        if float(k) >= x:
            correct += float(c)
        total += float(c)
    for k, c in zip(fk, fc):
        if float(k) < x:
            correct += float(c)
        total += float(c)
    return correct / total if total else math.nan


def scalar_evaluate(data, as_written=False):
    tk, tc, fk, fc = [np.asarray(a).tolist() for a in data]
    if not tk or not fk:
        return 0.5
    tp_sum = fp_sum = auc = 0.0
    t = 0
    for f in range(len(fk)):
        fp_v = fc[f]
        while t < len(tk) and (tc[t] <= fp_v if as_written else tk[t] <= fk[f]):
            tp_sum += float(tc[t])
            t += 1
        fp_sum += float(fp_v)
        auc += tp_sum * float(fp_v)
    while t < len(tk):
        tp_sum += float(tc[t])
        t += 1
    auc = _div(_div(auc, tp_sum), fp_sum)
    return 1 - auc if auc < .5 else auc


def _div(a, b):
    """a / b as IEEE 754 has it (Python raises where b is 0): the sums are 0
    when a side holds nothing but zero counts, which the reference's map may."""
    if b != 0:
        return a / b
    return math.nan if a == 0 or a != a else math.copysign(math.inf, a)


def scalar_exact(y, predict):
    y, p = np.asarray(y, F64).tolist(), np.asarray(predict, F64).tolist()
    order = sorted(range(len(p)), key=lambda i: p[i])  # stable; -0.0 == +0.0
    area = cum_tp = 0.0
    for i in order:
        if y[i] > 0:
            cum_tp += 1
        else:
            area += cum_tp
    d = cum_tp * (len(p) - cum_tp)
    if d == 0:
        return math.nan if area == 0 else math.inf
    area /= d
    return 1 - area if area < 0.5 else area


# ------------------------------------------------------------------ vector --
def _fold(terms):
    return np.add.accumulate(np.concatenate([[0.0], np.asarray(terms, F64)]))


def vector_keys(predict, goodness):
    with np.errstate(all="ignore"):
        prod = np.asarray(predict, F64) * F64(goodness)
        bad = ~(np.abs(prod) < 2.0 ** 63)
        return np.where(bad, I64(INT64_MIN), np.trunc(np.where(bad, 0.0, prod)).astype(I64))


def vector_compute(y, predict, goodness):
    k = vector_keys(predict, goodness)
    pos = np.asarray(y, F64) > 0
    tk, tc = np.unique(k[pos], return_counts=True)
    fk, fc = np.unique(k[~pos], return_counts=True)
    return tk.astype(I64), tc.astype(U64), fk.astype(I64), fc.astype(U64)


def _vector_side(keys, counts):
    keys = np.concatenate([np.asarray(k, I64) for k in keys] + [np.zeros(0, I64)])
    counts = np.concatenate([np.asarray(c, U64) for c in counts] + [np.zeros(0, U64)])
    keep = counts != 0
    uk, inv = np.unique(keys[keep], return_inverse=True)
    out = np.zeros(uk.size, U64)
    np.add.at(out, inv, counts[keep])
    return uk.astype(I64), out


def vector_merge(datas):
    tk, tc = _vector_side([d[0] for d in datas], [d[1] for d in datas])
    fk, fc = _vector_side([d[2] for d in datas], [d[3] for d in datas])
    return tk, tc, fk, fc


def vector_accuracy(data, goodness, threshold=0.0):
    tk, tc, fk, fc = data
    x = F64(threshold) * F64(goodness)
    cnt = np.concatenate([tc.astype(F64), fc.astype(F64)])
    right = np.concatenate([tk.astype(F64) >= x, fk.astype(F64) < x])
    with np.errstate(all="ignore"):
        return float(_fold(np.where(right, cnt, 0.0))[-1] / _fold(cnt)[-1])


def vector_evaluate(data, as_written=False):
    tk, tc, fk, fc = data
    if tk.size == 0 or fk.size == 0:
        return 0.5
    cum = _fold(tc.astype(F64))  # cum[t] = tp_sum after t positives' entries
    if as_written:
        taken, t = np.zeros(fk.size, np.int64), 0
        for f in range(fk.size):  # the pointer only moves forward
            later = np.nonzero(tc[t:] > fc[f])[0]
            t = t + int(later[0]) if later.size else tk.size
            taken[f] = t
    else:
        taken = np.searchsorted(tk, fk, side="right")
    auc = _fold(cum[taken] * fc.astype(F64))[-1]
    with np.errstate(all="ignore"):  # 0 / 0 where a side holds only zero counts
        auc = auc / cum[-1] / _fold(fc.astype(F64))[-1]
    return float(1 - auc if auc < .5 else auc)


def vector_exact(y, predict):
    y, p = np.asarray(y, F64), np.asarray(predict, F64)
    order = np.argsort(p, kind="stable")
    pos = y[order] > 0
    before = np.cumsum(pos) - pos  # positives sorted before each example
    a, npos = int(before[~pos].sum()), int(pos.sum())
    with np.errstate(all="ignore"):
        area = F64(a) / (F64(npos) * F64(p.size - npos))
    return float(1 - area if area < 0.5 else area)


# ------------------------------------------------------------------- cases --
LABELS = np.array([1.0, -1.0, 0.0, -0.0, np.nan, 2.5])


def mixed_labels(rng, n):
    return LABELS[rng.integers(0, LABELS.size, n)]


def sizes(tile):
    return (("1", 1), ("Tm1", tile - 1), ("T", tile), ("Tp1", tile + 1), ("3Tp5", 3 * tile + 5))


def add_cases(tile):
    """name -> (y, predict, goodness) around the sort tile `tile`."""
    rng = np.random.default_rng(41)
    big = 3 * tile + 5
    cases = {}
    special = np.array([0.4, -0.4, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 9.3e18,
                        -9.3e18, 2.0 ** 63, -2.0 ** 63, 0.99999, -0.99999, 1e-310])
    for name, n in sizes(tile):
        for g in (1, 10, 100000):
            p = rng.normal(0, 3, n)
            at = rng.permutation(n)[:min(n, special.size)]
            p[at] = special[:at.size]
            cases["mixed_%s_g%d" % (name, g)] = (mixed_labels(rng, n), p, g)
    cases["distinct"] = (mixed_labels(rng, big), (rng.permutation(big) - big // 2) * 2.0 + 0.5, 1)
    cases["one_key"] = (mixed_labels(rng, big), np.full(big, 0.123), 10)
    seam = np.sort(rng.integers(-40, 40, big)).astype(F64)
    seam[tile - 7:tile + 9] = seam[tile]  # one run across the first seam
    seam = np.sort(seam)
    cases["seam_run"] = (mixed_labels(rng, big), seam, 1)
    return cases


def exact_cases(tile):
    """name -> (y, predict): no NaN prediction, both classes unless named."""
    rng = np.random.default_rng(43)
    big = 3 * tile + 5
    cases = {}
    for name, n in sizes(tile):
        cases["distinct_%s" % name] = (mixed_labels(rng, n), rng.permutation(n) * 0.5 - n / 4)
    ties = np.sort(rng.integers(-9, 9, big)).astype(F64)
    ties[tile - 5:tile + 5] = ties[tile]
    cases["ties_seam"] = (mixed_labels(rng, big), np.sort(ties))
    cases["ties_shuffled"] = (mixed_labels(rng, big), rng.integers(-9, 9, big).astype(F64))
    cases["zeros_pos_first"] = (np.array([1.0, -1.0]), np.array([-0.0, 0.0]))
    cases["zeros_neg_first"] = (np.array([-1.0, 1.0]), np.array([-0.0, 0.0]))
    cases["zeros_reversed"] = (np.array([1.0, -1.0]), np.array([0.0, -0.0]))
    odd = rng.normal(0, 1, big)
    odd[:8] = [-np.inf, np.inf, 5e-324, -5e-324, 1e-310, -1e-310, -0.0, 0.0]
    odd[8:200] = -np.abs(odd[8:200]) * 1e-300
    cases["signs_denormals_inf"] = (mixed_labels(rng, big), rng.permutation(odd))
    cases["all_positive"] = (np.ones(tile + 1), rng.normal(0, 1, tile + 1))
    cases["all_negative"] = (-np.ones(tile + 1), rng.normal(0, 1, tile + 1))
    return cases
