"""CPU restatements of the reference's online model, for the FTRL tests.

Two independent forms of ``FTRLModel<K, double>::setValue`` (reference
src/linear_method/ftrl_model.h:80-112 with grad_norm :60-63 and
base/soft_thresholding.h:7-13):

``ScalarFTRL``  one key after the other with Python floats (IEEE binary64,
                one correctly rounded operation per Python operator);
``VectorFTRL``  one message at a time in numpy float64.  The keys of one
                message are distinct, so they are independent and the
                vector form is exact, not an approximation.

Both keep the reference's bookkeeping (nnz, the four kinds of weight
transition) and neither checks its input, as the reference does not.

PINNED: tests/test_reference_pin.py holds both classes, with ``pull``,
``nonzero`` and ``dump_text``, bit for bit to what the reference's own
ftrl_model.h (compiled in place, oracle/ref_ftrl_shim.cc) gave on the
recorded case (tests/golden/reference_pin/ftrl_*.npz) and, where oracle/_ref
is built, gives on seeded cases.  The norms are not restated here (a defined
deviation of the product, include/psg.h).
"""
import math

import numpy as np

TRANSITIONS = ("zero_nonzero", "nonzero_zero", "zero_zero", "nonzero_nonzero")


def bits(a):
    """The bit patterns of a float64 array (so -0.0 != +0.0, NaN == NaN)."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _grad_norm(pos, neg):  # ftrl_model.h:60-63: the counts become V first
    p, n = float(pos), float(neg)
    al = p + n
    return 0.0 if al == 0 else math.sqrt(p * n / al)


def _soft_thresholding(x, l1, l2):  # soft_thresholding.h:7-13, comparisons as written
    if x > 0:
        return (x - l1) / l2 if x > l1 else 0.0
    else:
        return (x + l1) / l2 if x < -l1 else 0.0


def _kind(w, w_old):
    return ("zero_" if w_old == 0 else "nonzero_") + ("zero" if w == 0 else "nonzero")


class ScalarFTRL:
    def __init__(self, alpha, beta, lambda1, lambda2):
        self.alpha, self.beta = float(alpha), float(beta)
        self.lambda1, self.lambda2 = float(lambda1), float(lambda2)
        self.model = {}  # key -> [pos, neg, w, z]
        self.nnz = 0
        self.transitions = dict.fromkeys(TRANSITIONS, 0)

    def push(self, keys, pos, neg, grad):
        for k, dp, dn, g in zip(np.asarray(keys).tolist(), np.asarray(pos).tolist(),
                                np.asarray(neg).tolist(), np.asarray(grad).tolist()):
            e = self.model.setdefault(k, [0, 0, 0.0, 0.0])
            sqrt_n = _grad_norm(e[0], e[1])
            e[0] = (e[0] + dp) & 0xFFFFFFFFFFFFFFFF
            e[1] = (e[1] + dn) & 0xFFFFFFFFFFFFFFFF
            sqrt_n_new = _grad_norm(e[0], e[1])
            sigma = (sqrt_n_new - sqrt_n) / self.alpha
            e[3] = e[3] + (g - sigma * e[2])
            lambda2 = self.lambda2 + (self.beta + sqrt_n_new) / self.alpha
            w_old = e[2]
            w = -_soft_thresholding(e[3], self.lambda1, lambda2)
            e[2] = w
            if w == 0 and w_old != 0:
                self.nnz -= 1
            elif w != 0 and w_old == 0:
                self.nnz += 1
            self.transitions[_kind(w, w_old)] += 1

    @property
    def entries(self):
        return len(self.model)

    def lookup(self, keys):
        keys = np.asarray(keys, np.uint64)
        pos, neg = np.zeros(keys.size, np.uint64), np.zeros(keys.size, np.uint64)
        w, z = np.zeros(keys.size, np.float64), np.zeros(keys.size, np.float64)
        found = np.zeros(keys.size, np.uint8)
        for i, k in enumerate(keys.tolist()):
            e = self.model.get(k)
            if e is not None:
                pos[i], neg[i], w[i], z[i], found[i] = e[0], e[1], e[2], e[3], 1
        return pos, neg, w, z, found


class VectorFTRL:
    def __init__(self, alpha, beta, lambda1, lambda2):
        self.alpha, self.beta = np.float64(alpha), np.float64(beta)
        self.lambda1, self.lambda2 = np.float64(lambda1), np.float64(lambda2)
        self.keys = np.zeros(0, np.uint64)  # sorted
        self.pos, self.neg = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        self.w, self.z = np.zeros(0, np.float64), np.zeros(0, np.float64)
        self.nnz = 0
        self.transitions = dict.fromkeys(TRANSITIONS, 0)

    @staticmethod
    def _grad_norm(pos, neg):
        p, n = pos.astype(np.float64), neg.astype(np.float64)
        al = p + n
        with np.errstate(all="ignore"):
            return np.where(al == 0, 0.0, np.sqrt(p * n / al))

    def push(self, keys, pos, neg, grad):
        keys = np.asarray(keys, np.uint64)
        if keys.size == 0:
            return
        allk = np.union1d(self.keys, keys)
        if allk.size != self.keys.size:
            at = np.searchsorted(allk, self.keys)
            for name in ("pos", "neg", "w", "z"):
                old = getattr(self, name)
                new = np.zeros(allk.size, old.dtype)
                new[at] = old
                setattr(self, name, new)
            self.keys = allk
        i = np.searchsorted(self.keys, keys)
        with np.errstate(all="ignore"):
            sqrt_n = self._grad_norm(self.pos[i], self.neg[i])
            self.pos[i] += np.asarray(pos, np.uint32).astype(np.uint64)
            self.neg[i] += np.asarray(neg, np.uint32).astype(np.uint64)
            sqrt_n_new = self._grad_norm(self.pos[i], self.neg[i])
            sigma = (sqrt_n_new - sqrt_n) / self.alpha
            w_old = self.w[i]
            z = self.z[i] + (np.asarray(grad, np.float64) - sigma * w_old)
            lambda2 = self.lambda2 + (self.beta + sqrt_n_new) / self.alpha
            st = np.where(z > 0,
                          np.where(z > self.lambda1, (z - self.lambda1) / lambda2, 0.0),
                          np.where(z < -self.lambda1, (z + self.lambda1) / lambda2, 0.0))
            w = np.negative(st)
        self.z[i] = z
        self.w[i] = w
        was, now = w_old != 0, w != 0
        self.nnz += int(np.count_nonzero(now & ~was)) - int(np.count_nonzero(~now & was))
        self.transitions["zero_nonzero"] += int(np.count_nonzero(~was & now))
        self.transitions["nonzero_zero"] += int(np.count_nonzero(was & ~now))
        self.transitions["zero_zero"] += int(np.count_nonzero(~was & ~now))
        self.transitions["nonzero_nonzero"] += int(np.count_nonzero(was & now))

    @property
    def entries(self):
        return int(self.keys.size)

    def lookup(self, keys):
        keys = np.asarray(keys, np.uint64)
        pos, neg = np.zeros(keys.size, np.uint64), np.zeros(keys.size, np.uint64)
        w, z = np.zeros(keys.size, np.float64), np.zeros(keys.size, np.float64)
        found = np.zeros(keys.size, np.uint8)
        if self.keys.size and keys.size:
            i = np.minimum(np.searchsorted(self.keys, keys), self.keys.size - 1)
            hit = self.keys[i] == keys
            j = i[hit]
            pos[hit], neg[hit], w[hit], z[hit], found[hit] = \
                self.pos[j], self.neg[j], self.w[j], self.z[j], 1
        return pos, neg, w, z, found


def pull(model, keys):
    """getValue: w of each key, +0.0 for one never pushed."""
    return model.lookup(keys)[2]


def nonzero(model, universe):
    """writeToFile's entries among `universe`: (keys, w) with w != 0, by key."""
    u = np.unique(np.asarray(universe, np.uint64))
    w = model.lookup(u)[2]
    keep = w != 0
    return u[keep], w[keep]


def dump_text(model, universe):
    """The text of writeToFile, sorted by key: ``key\\tw`` with w as the
    default ostream prints a double (%g)."""
    k, w = nonzero(model, universe)
    return "".join("%d\t%s\n" % (a, "%g" % b) for a, b in zip(k.tolist(), w.tolist()))


PARITY_PARAM = dict(alpha=1.0, beta=1.0, lambda1=1.0, lambda2=0.1)


def parity_case(seed=1, nmsg=6, n=1200, universe=3000):
    """The parity case: nmsg messages of n keys drawn without replacement
    from `universe` scattered keys; pos, neg uniform in 0..5; grad = 2 N(0,1).
    Returns (universe keys sorted, [(keys, pos, neg, grad)])."""
    rng = np.random.default_rng(seed)
    uni = np.unique(rng.integers(0, 1 << 63, size=universe + 64, dtype=np.uint64))[:universe]
    assert uni.size == universe
    msgs = []
    for _ in range(nmsg):
        k = np.sort(rng.choice(uni, size=n, replace=False))
        msgs.append((k, rng.integers(0, 6, size=n).astype(np.uint32),
                     rng.integers(0, 6, size=n).astype(np.uint32),
                     2.0 * rng.standard_normal(n)))
    return uni, msgs


def absent_keys(universe, n, seed=7):
    """n keys that are not in `universe`."""
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(0, 1 << 64, size=2 * n + 16, dtype=np.uint64))
    c = c[~np.isin(c, universe)]
    assert c.size >= n
    return rng.permutation(c)[:n]
