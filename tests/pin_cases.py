"""TEST INFRASTRUCTURE: the fixed inputs of the reference-pinning fixtures
(tests/golden/reference_pin/*.npz) and their loader.

tools/record_reference.py runs the reference's own code (oracle/_ref, built
from the reference tree by oracle/Makefile) on these inputs and stores what
it returns; tests/test_reference_pin.py (CPU) and the GPU tests rebuild the
same inputs here, check their SHA-256 against the fixture and compare bit for
bit.  Every input comes from splitmix64 in numpy uint64 arithmetic, never
from a library RNG, so a fixture does not depend on the numpy version.
Floats are integers scaled by a power of two, plus listed special values.
The inputs of the snappy fixtures (tests/golden/snappy_pin/*.npz, recorded
by tools/record_snappy.py from the real snappy compressor) are built here
too, the same way: snappy_cases().

What the inputs avoid, and why: two NaNs never meet in one add (which
payload survives is not fixed by IEEE 754) and +inf never meets -inf, nor
0 an infinity in a product (the default NaN's sign differs between x86 and
the GPU).  Everything else -- -0.0, single NaNs quiet and signalling, +-inf,
denormals, 0xFFFFFFFF counts -- is in.  The AUC and localizer cases add no
float arithmetic of their own to what is recorded: keys, counts and indices
are integers, values are copied, and a 0 / 0 result is compared as "a NaN".
An output of more than ARRAY_CAP bytes is recorded as its SHA-256 only
(record_output / same_output).
"""
import hashlib
import json
import math
import os
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pin")
U64 = (1 << 64) - 1
_u = np.uint64
_GAMMA = 0x9E3779B97F4A7C15


# ------------------------------------------------------------ integer mixing
def splitmix64(seed, n):
    """The first n outputs of splitmix64 seeded with `seed` (uint64 array)."""
    with np.errstate(over="ignore"):
        z = _u(seed & U64) + (np.arange(1, n + 1, dtype=np.uint64) * _u(_GAMMA))
        z = (z ^ (z >> _u(30))) * _u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _u(27))) * _u(0x94D049BB133111EB)
        return z ^ (z >> _u(31))


def fmix64(k):
    """MurmurHash3's finaliser, the FTRL table's hash (psg_ftrl.hip)."""
    k = np.asarray(k, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> _u(33)
        k *= _u(0xff51afd7ed558ccd)
        k ^= k >> _u(33)
        k *= _u(0xc4ceb9fe1a85ec53)
        k ^= k >> _u(33)
    return k


_INV1 = pow(0xff51afd7ed558ccd, -1, 1 << 64)
_INV2 = pow(0xc4ceb9fe1a85ec53, -1, 1 << 64)


def unmix64(h):
    """fmix64's inverse: x ^= x >> 33 is its own inverse (33 >= 32), and the
    two odd multipliers have inverses mod 2^64."""
    h = np.asarray(h, np.uint64).copy()
    with np.errstate(over="ignore"):
        h ^= h >> _u(33)
        h *= _u(_INV2)
        h ^= h >> _u(33)
        h *= _u(_INV1)
        h ^= h >> _u(33)
    return h


def chance(x, p):
    """x (uint64 draws) as Bernoulli(p), in integer arithmetic."""
    return (x >> _u(32)) < _u(int(p * (1 << 32)))


def scaled(x, dtype):
    """Draws as floats: an integer scaled by a power of two.  f32: 24-bit
    signed integers / 2^12, f64: 53-bit signed integers / 2^40 (sums of a few
    of them need more bits than the format has, so the fold order shows)."""
    if np.dtype(dtype) == np.float32:
        return ((x >> _u(40)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 12)
    return ((x >> _u(11)).astype(np.int64) - (1 << 52)).astype(np.float64) / np.float64(1 << 40)


def unique_keys(seed, n):
    """n distinct sorted keys over the whole uint64 range, none 2^64 - 1
    (Range::all() ends there)."""
    k = np.unique(splitmix64(seed, n + 64))
    k = k[k != _u(U64)]
    assert k.size >= n
    return np.ascontiguousarray(k[np.sort(np.argsort(splitmix64(seed + 1, k.size), kind="stable")[:n])])


def sha256(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes())
    return h.hexdigest()


def fbits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------ fold cases
def _from_bits(b, dtype):
    ut = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    return np.array([b], ut).view(dtype)[0]


class FoldCase:
    """D, pushes [(keys, [vals] * m)], the key ranges it is recorded over,
    a gather (server values W, request R) and the name of its fixtures."""

    def __init__(self, name, dtype, m, D, pushes, ranges, W, R):
        self.name, self.dtype, self.m = name, np.dtype(dtype), m
        self.D, self.pushes, self.ranges, self.W, self.R = D, pushes, ranges, W, R

    def fixture(self, r):
        return "fold_%s_r%d" % (self.name, r)

    def sliced(self, r):
        """The pushes cut to key range r, as sliceKeyOrderedMsg hands them to
        the server that owns it; empty ones never reach it."""
        kb, ke = self.ranges[r]
        out = []
        for k, vs in self.pushes:
            keep = (k >= _u(kb)) & (k < _u(ke))
            if keep.any():
                out.append((np.ascontiguousarray(k[keep]),
                            [np.ascontiguousarray(v[keep]) for v in vs]))
        return out

    def digest(self):
        arrs = [self.D, self.W, self.R, np.array(self.ranges, np.uint64).ravel()]
        for k, vs in self.pushes:
            arrs += [k] + [fbits(v) for v in vs]
        return sha256(arrs)


def _gather_inputs(seed, D, dtype):
    W = scaled(splitmix64(seed, D.size), dtype)
    W[::97] = -0.0
    pick = D[chance(splitmix64(seed + 1, D.size), 0.1)]
    absent = pick[:100] + _u(1)
    absent = absent[~np.isin(absent, D)]
    R = np.sort(np.concatenate([pick, absent, pick[5:55]]))  # 50 keys twice
    return W, np.ascontiguousarray(R)


def fold_case(name):
    if name == "F1":
        # f32, m = 1: 5,000 keys = five 1024-slot tiles / three 2048-slot
        # tiles, the last partial; 70 pushes keep each key with p = 0.3
        # (push groups 32+32+6 or 64+6); -0.0 in 5 % of the values, and in
        # every value of one slot in 64 (a slot of the first push stays -0.0
        # under parallelSetValue and turns +0.0 under serialSetValue)
        dtype, m, nD = np.float32, 1, 5000
        D = unique_keys(101, nD)
        pushes = []
        for p in range(70):
            keep = chance(splitmix64(1000 + p, nD), 0.3)
            k = D[keep]
            v = scaled(splitmix64(2000 + p, k.size), dtype)
            v[chance(splitmix64(3000 + p, k.size), 0.05)] = -0.0
            v[np.nonzero(keep)[0] % 64 == 5] = -0.0  # slots that only ever see -0.0
            pushes.append((k, [v]))
        ranges = [(0, U64)]
    elif name == "F2":
        # f64, m = 2: 2,049 keys (one past a tile seam), 9 pushes
        dtype, m, nD = np.float64, 2, 2049
        D = unique_keys(201, nD)
        sel = [np.array([0]), np.array([nD - 1]), np.arange(nD), np.arange(1024, 2048)]
        mid = np.arange(1500, nD)
        sel.append(mid[chance(splitmix64(1204, mid.size), 0.5)])  # starts mid-tile
        for p in range(5, 9):
            sel.append(np.nonzero(chance(splitmix64(1200 + p, nD), 0.4))[0])
        # special values, each on a slot of its own (slot -> bits), carried by
        # push 2 (every key) only; other pushes hold finite values there
        special = {40: 0x7ff8000000001234,    # quiet NaN with a payload
                   900: 0x7ff0000000000abc,   # signalling NaN with a payload
                   1023: 0x7ff0000000000000,  # +inf on the last slot of tile 0
                   1024: 0xfff0000000000000,  # -inf on the first slot of tile 1
                   1700: 0x0000000000000003,  # a denormal
                   2048: 0x8000000000000001}  # a negative denormal, last slot
        zero_slots = np.array([0, 7, 1025, 2047])  # -0.0 in EVERY push holding them
        pushes = []
        for p, s in enumerate(sel):
            vs = []
            for i in range(m):
                v = scaled(splitmix64(2200 + 10 * p + i, s.size), dtype)
                v[np.isin(s, zero_slots)] = -0.0
                if p == 2:
                    for slot, b in special.items():
                        # value array 1 carries them with the other sign
                        v[slot] = _from_bits(b if i == 0 else b ^ (1 << 63), dtype)
                vs.append(v)
            pushes.append((D[s], vs))
        ranges = [(0, U64), (int(D[700]), int(D[1800]))]  # both ends mid-tile
    elif name == "F3":
        # f32, m = 1: 6,000 keys, 150 pushes of 1 to 40 keys (packed form)
        dtype, m, nD = np.float32, 1, 6000
        D = unique_keys(301, nD)
        size = 1 + (splitmix64(1300, 150) % _u(40)).astype(np.int64)
        pushes = []
        slots = [np.sort(np.argsort(splitmix64(1400 + p, nD), kind="stable")[: size[p]])
                 for p in range(150)]
        first = slots[0][:3]  # the first push's first three slots
        for p, idx in enumerate(slots):
            v = scaled(splitmix64(2400 + p, idx.size), dtype)
            v[chance(splitmix64(3400 + p, idx.size), 0.05)] = -0.0
            v[(idx % 64 == 5) | np.isin(idx, first)] = -0.0  # slots that only ever see -0.0
            pushes.append((D[idx], [v]))
        ranges = [(0, U64)]
    else:
        raise KeyError(name)
    W, R = _gather_inputs(hash_name(name), D, dtype)
    return FoldCase(name, dtype, m, D, pushes, ranges, W, R)


def hash_name(name):
    return 5000 + 100 * int(name[1:])


FOLD_NAMES = ("F1", "F2", "F3")
EVEN_DIVIDE_N = (1, 2, 3, 7, 8, 16)


def random_fold_case(seed):
    """Seeded cases beyond the fixtures (live tests): dtype, m = 1..3, a
    sub-range on the odd seeds."""
    dtype = np.float32 if seed % 2 == 0 else np.float64
    m = 1 + seed % 3
    nD = [3000, 1025, 4096, 2500, 777, 5001, 2048, 1][seed % 8]
    npush = [5, 33, 2, 70, 9, 12, 65, 3][seed % 8]
    dens = [0.5, 0.1, 1.0, 0.05, 0.3, 0.02, 0.2, 1.0][seed % 8]
    D = unique_keys(7000 + seed, nD)
    pushes = []
    for p in range(npush):
        keep = chance(splitmix64(7100 + 100 * seed + p, nD), dens)
        k = D[keep]
        vs = []
        for i in range(m):
            v = scaled(splitmix64(7200 + 1000 * seed + 10 * p + i, k.size), dtype)
            v[chance(splitmix64(7300 + 1000 * seed + 10 * p + i, k.size), 0.1)] = -0.0
            vs.append(v)
        pushes.append((k, vs))
    ranges = [(0, U64)]
    if seed % 2 == 1 and nD > 8:
        ranges = [(int(D[nD // 5]), int(D[-(nD // 7)]))]
    W, R = _gather_inputs(7400 + seed, D, dtype)
    return FoldCase("R%d" % seed, dtype, m, D, pushes, ranges, W, R)


# ------------------------------------------------------------------- FTRL cases
FTRL_PARAMS = {"parity": dict(alpha=1.0, beta=1.0, lambda1=1.0, lambda2=0.1),
               "steep": dict(alpha=0.05, beta=1.0, lambda1=0.5, lambda2=0.0)}
LOW24 = (1 << 24) - 1


class FtrlCase:
    def __init__(self, keys, last_bucket, bucket0, msgs, request, inf_keys):
        self.keys, self.last_bucket, self.bucket0 = keys, last_bucket, bucket0
        self.msgs, self.request, self.inf_keys = msgs, request, inf_keys

    def digest(self):
        arrs = [self.keys, self.request]
        for k, p, n, g in self.msgs:
            arrs += [k, p, n, fbits(g)]
        return sha256(arrs)

    def finite_msgs(self):
        """The messages without the two keys whose gradient is infinite (their
        weights are, and the reference's norms and objv with them)."""
        out = []
        for k, p, n, g in self.msgs:
            keep = ~np.isin(k, self.inf_keys)
            out.append((k[keep], p[keep], n[keep], g[keep]))
        return out


def ftrl_case(seed=0, nscatter=1200, nmsg=6):
    """About 1,500 keys: scattered ones; 0 and 2^64 - 1; 16 differing only
    above bit 58; 60 whose fmix64 has its low 24 bits all ones (the last
    bucket of every table up to 2^24 buckets) and 60 whose fmix64 has them
    zero (bucket 0, where the wrapped chain collides with them).  Six
    strictly increasing messages of about 600 keys; the first carries every
    crowded key, 0, 2^64 - 1 and the 16; some scattered keys are in none."""
    s = 9000 + 1000 * seed
    scattered = unique_keys(s, nscatter)
    high = _u(0x02AAAAAAAAAAAAAA) | (np.arange(16, dtype=np.uint64) << _u(60))
    hi = splitmix64(s + 2, 120) & ~_u(LOW24)
    last_bucket = unmix64(hi[:60] | _u(LOW24))
    bucket0 = unmix64(hi[60:])
    keys = np.unique(np.concatenate([scattered, np.array([0, U64], np.uint64), high,
                                     last_bucket, bucket0]))
    assert keys.size == nscatter + 2 + 16 + 120
    crowded = np.isin(keys, np.concatenate([last_bucket, bucket0, high,
                                            np.array([0, U64], np.uint64)]))
    # fixed keys (scattered ones, by position): 0xFFFFFFFF counts on three,
    # special gradients on five
    big = scattered[np.array([10, 500, 1100]) * nscatter // 1200]
    g_nan, g_pinf, g_ninf, g_nzero, g_den = scattered[np.array([20, 300, 600, 900, 1150]) * nscatter // 1200]
    msgs = []
    for t in range(nmsg):
        keep = chance(splitmix64(s + 10 + t, keys.size), 0.42)
        if t == 0:
            keep |= crowded
        k = np.ascontiguousarray(keys[keep])
        n = k.size
        pos = (splitmix64(s + 20 + t, n) % _u(6)).astype(np.uint32)
        neg = (splitmix64(s + 30 + t, n) % _u(6)).astype(np.uint32)
        grad = ((splitmix64(s + 40 + t, n) >> _u(11)).astype(np.int64)
                - (1 << 52)).astype(np.float64) / np.float64(1 << 50)  # [-4, 4)
        isbig = np.isin(k, big)
        pos[isbig] = neg[isbig] = 0xFFFFFFFF
        grad[k == g_nan] = np.nan
        grad[k == g_pinf] = np.inf
        grad[k == g_ninf] = -np.inf
        grad[k == g_nzero] = -0.0
        grad[k == g_den] = 5e-324
        # an infinite weight times sigma = 0 would be the default NaN: the
        # infinite-gradient keys' counts grow in every message, so sigma > 0
        isinf = (k == g_pinf) | (k == g_ninf)
        pos[isinf] = neg[isinf] = 1
        msgs.append((k, pos, neg, grad))
    absent = fmix64(splitmix64(s + 50, 200))
    absent = absent[~np.isin(absent, keys)]
    req = np.concatenate([keys, absent, keys[:99]])
    req = np.ascontiguousarray(req[np.argsort(splitmix64(s + 51, req.size), kind="stable")])
    return FtrlCase(keys, last_bucket, bucket0, msgs, req, np.array([g_pinf, g_ninf], np.uint64))


def objv_interval(w, entries, lambda1, lambda2):
    """The interval psg.h's bound leaves objv: norm1 within entries * 2^-53 *
    (the exact sum |w|) of it, norm2 likewise of the exact sum w^2, objv
    increasing in both; plus 2 ulp for the four roundings of
    norm1 * lambda1 + .5 * lambda2 * sqrt(norm2) itself."""
    getcontext().prec = 80
    s1 = sum(Fraction(abs(x)) for x in w)
    s2 = sum(Fraction(x) * Fraction(x) for x in w)
    eps = Fraction(entries, 1 << 53)

    def objv(n1, n2):
        root = (Decimal(n2.numerator) / Decimal(n2.denominator)).sqrt()
        return float(Decimal(n1.numerator) / Decimal(n1.denominator) * Decimal(lambda1)
                     + Decimal(0.5) * Decimal(lambda2) * root)
    lo, hi = objv(s1 * (1 - eps), s2 * (1 - eps)), objv(s1 * (1 + eps), s2 * (1 + eps))
    return lo - 2 * math.ulp(lo), hi + 2 * math.ulp(hi)


def entry_digest(pos, neg, w, z, found):
    return sha256([np.asarray(pos, np.uint64), np.asarray(neg, np.uint64),
                   fbits(np.asarray(w, np.float64)), fbits(np.asarray(z, np.float64)),
                   np.asarray(found, np.uint8)])


def sorted_dump(text):
    """writeToFile's lines sorted by key."""
    lines = [ln for ln in text.split("\n") if ln]
    lines.sort(key=lambda ln: int(ln.split("\t")[0]))
    return "".join(ln + "\n" for ln in lines)


# --------------------------------------------------------------- CountMin cases
CM_SHAPES = ((10, 3), (1000, 1), (777, 40), (65537, 4))
CM_FREQS = (0, 3, 100, 254)


class CmCase:
    def __init__(self, n, k, batches, query):
        self.n, self.k, self.batches, self.query = n, k, batches, query

    def digest(self):
        arrs = [np.array([self.n, self.k], np.int64), self.query]
        for k, c in self.batches:
            arrs += [k, c]
        return sha256(arrs)


def cm_case(n, k, seed=0):
    """Three insertKeys batches of 2,000 unique keys out of 6,000 with counts
    up to 700 (byte wrap), and a 3,000-key query with repeats and keys never
    inserted."""
    s = 20000 + 1000 * seed + 7 * n + k
    uni = unique_keys(s, 6000)
    batches = []
    for b in range(3):
        idx = np.sort(np.argsort(splitmix64(s + 10 + b, uni.size), kind="stable")[:2000])
        counts = (splitmix64(s + 20 + b, 2000) % _u(701)).astype(np.uint32)
        batches.append((np.ascontiguousarray(uni[idx]), counts))
    query = np.ascontiguousarray(uni[(splitmix64(s + 30, 3000) % _u(uni.size)).astype(np.int64)])
    return CmCase(n, k, batches, query)


# ------------------------------------------------------------------ AUC cases
# Inputs of auc.npz, auc_merge.npz and exact_auc.npz (reference src/base/auc.h,
# src/base/evaluation.h).  The sizes sit around the device sort's tile
# (psg_mb_sort_tile(), 256 * PSG_SORT_KPT pairs): PIN_TILE is its value when
# the fixtures were recorded and is stored in their meta; the GPU tests assert
# that the library still has it.
PIN_TILE = 2048
AUC_GOODNESS = (1, 10, 100, 1000, 100000, -1000)
AUC_LABELS = np.array([1.0, -1.0, 0.0, -0.0, 0.5, 2.0, np.nan])  # > 0 is a positive: 1, 0.5, 2
AUC_THRESHOLDS = (0.0, 0.5, -0.25)
ARRAY_CAP = 8192  # a recorded output of more bytes is stored as its SHA-256 only
# decimals whose product with a power of ten rounds onto an integer or just
# below one (0.29 * 100 = 28.999999999999996 -> key 28, 0.57 * 100 =
# 56.99999999999999, 4.35 * 100 = 434.99999999999994; 0.7 * 10 = 7 and
# 0.1 * 10 = 1 exactly, though neither factor is)
_DECIMALS = (0.29, 0.7, 0.1, 0.029, 0.007, 0.001, 0.00029, 0.00007, 0.00001, 0.57, 0.58, 4.35,
             1.15, 8.2, 2.675, 0.3, 0.6, 0.9, 1.1, 16.08, 0.0003, 0.019999999999999997)


def pin_sizes(tile=PIN_TILE):
    return (1, tile - 1, tile, tile + 1, 3 * tile + 5)


def spread20(x):
    """Draws as doubles in [-20, 20): an integer / 2^30."""
    return ((x % _u(40 << 30)).astype(np.int64) - (20 << 30)).astype(np.float64) / np.float64(1 << 30)


def auc_labels(seed, n):
    return AUC_LABELS[(splitmix64(seed, n) % _u(AUC_LABELS.size)).astype(np.int64)]


def _place(seed, base, special):
    """base with the first min(n, m) of `special` at drawn positions."""
    at = np.argsort(splitmix64(seed, base.size), kind="stable")[:min(base.size, special.size)]
    base[at] = special[:at.size]
    return base


def auc_specials(g):
    """Predictions whose key under goodness g is DEFINED and easy to get
    wrong: decimals around an integer product, negatives in (-1/|g|, 0)
    (truncation toward zero gives key 0, not -1), both zeros, denormals, and
    +-1e18 / |g| (exact, so the product is +-1e18 < 2^63).  With g = 1 also the
    largest doubles below 2^63 in magnitude."""
    a = float(abs(g))
    dec = np.array(_DECIMALS)
    inside = np.array([-0.5, -0.999, -(2.0 ** -30)]) / a
    out = [dec[:1], -dec[:1], inside, -inside, dec[1:], -dec[1:],
           np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e18 / a, -1e18 / a])]
    if g == 1:
        out.append(np.array([2.0 ** 63 - 1024, -(2.0 ** 63 - 1024), 2.0 ** 62, -(2.0 ** 62)]))
    return np.concatenate(out)


def auc_undefined(g):
    """Predictions whose product with g has no defined conversion to int64 in
    C++ (NaN, or of magnitude >= 2^63; -2^63 itself is counted here too, as
    psg.h counts it)."""
    a = float(abs(g))
    return np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 9.3e18 / a, -9.3e18 / a, 1e19 / a,
                     -1e19 / a, 2.0 ** 63 / a, -(2.0 ** 63) / a, 1.7976931348623157e308])


class AucCase:
    def __init__(self, name, y, p, g):
        self.name, self.y, self.p, self.g = name, y, p, g

    def digest(self):
        return sha256([fbits(self.y), fbits(self.p), np.array([self.g], np.int64)])


def auc_cases():
    """[AucCase]: every size with every goodness, defined conversions only;
    then one case per goodness (257 examples) that also holds the undefined
    ones, kept apart so that the defined cases stay clean."""
    out = []
    for i, n in enumerate(pin_sizes()):
        for j, g in enumerate(AUC_GOODNESS):
            s = 50000 + 100 * i + 10 * j
            p = _place(s + 2, spread20(splitmix64(s, n)), auc_specials(g))
            out.append(AucCase("n%d_g%d" % (n, g), auc_labels(s + 1, n), p, g))
    for j, g in enumerate(AUC_GOODNESS):
        s = 51000 + 10 * j
        p = _place(s + 2, spread20(splitmix64(s, 257)),
                   np.concatenate([auc_undefined(g), auc_specials(g)[:20]]))
        out.append(AucCase("undefined_g%d" % g, auc_labels(s + 1, 257), p, g))
    return out


def _auc_side(seed, n, universe, unique, shift=14):
    """n draws as (keys in [-universe/2, universe/2), counts below 2^(64 -
    shift)): with shift = 14 a few hundred counts sum past 2^53, so the order
    of accuracy's and evaluate's double sums shows."""
    k = (splitmix64(seed, n) % _u(universe)).astype(np.int64) - universe // 2
    if unique:
        k = np.unique(k)
    c = (splitmix64(seed + 1, k.size) >> _u(shift)) + _u(1)
    return np.ascontiguousarray(k), np.ascontiguousarray(c)


def auc_merge_sequences():
    """name -> (goodness, [AUCData]): what a root merges, then accuracy at
    AUC_THRESHOLDS and evaluate()."""
    seq = {}
    z64, zu = np.zeros(0, np.int64), np.zeros(0, np.uint64)
    # three workers' AUCData as compute writes them: ascending distinct keys
    seq["three_workers"] = (10, [_auc_side(52000 + 10 * w, 300, 400, True)
                                 + _auc_side(52005 + 10 * w, 300, 400, True) for w in range(3)])
    # unsorted lists that repeat keys, small counts among the large
    rep = []
    for w in range(2):
        tk, tc = _auc_side(52100 + 10 * w, 500, 60, False)
        fk, fc = _auc_side(52105 + 10 * w, 500, 60, False, shift=60)
        rep.append((tk, tc, fk, fc))
    seq["repeated_keys"] = (1000, rep)
    # zero counts: on keys that other entries also hit, and on keys (+-777777)
    # that only ever get a zero; both sides keep non-zero entries
    zc = []
    for w in range(3):
        tk, tc = _auc_side(52200 + 10 * w, 200, 300, w != 1, shift=50)
        fk, fc = _auc_side(52205 + 10 * w, 200, 300, w != 1, shift=50)
        tc[chance(splitmix64(52208 + 10 * w, tc.size), 0.3)] = 0
        fc[chance(splitmix64(52209 + 10 * w, fc.size), 0.3)] = 0
        only = np.array([777777, -777777], np.int64)
        zc.append((np.concatenate([tk, only]), np.concatenate([tc, np.zeros(2, np.uint64)]),
                   np.concatenate([fk, -only]), np.concatenate([fc, np.zeros(2, np.uint64)])))
    seq["zero_counts"] = (100, zc)
    # the boundary of "dropping zero counts changes no result": a side that
    # holds nothing but zero counts is not empty() in the reference
    tk, tc = _auc_side(52300, 50, 40, True, shift=60)
    seq["zero_only_negatives"] = (10, [(tk, tc, np.array([3, -7, 3], np.int64), np.zeros(3, np.uint64))])
    seq["zero_only_both"] = (10, [(np.array([1, 2], np.int64), np.zeros(2, np.uint64),
                                   np.array([0], np.int64), np.zeros(1, np.uint64))])
    # one side empty: evaluate is .5
    seq["no_negatives"] = (1000, [_auc_side(52400 + w, 100, 90, True) + (z64, zu) for w in range(2)])
    seq["no_positives"] = (-1000, [(z64, zu) + _auc_side(52450, 100, 90, True)])
    # accuracy compares (double)key with x = threshold * goodness: goodness
    # 2^55 puts x at 0, 2^54 and -2^53, where key +- 1 rounds onto x
    e54, e53 = 1 << 54, 1 << 53
    seq["keys_past_2p53"] = (1 << 55, [
        (np.array([-e53 - 1, -e53, -e53 + 1, e54 - 1, e54, e54 + 1, e54 + 3, 0, -1], np.int64),
         np.array([1, 2, 4, 8, 16, 32, 64, 128, 256], np.uint64),
         np.array([-e53 - 1, -e53, -e53 + 1, e54 - 1, e54, e54 + 1, e54 + 3, 0, -1,
                   -(1 << 63), (1 << 63) - 1], np.int64),
         np.array([3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37], np.uint64))])
    return seq


def auc_sequence_digest(goodness, datas):
    return sha256([np.array([goodness], np.int64)] + [a for d in datas for a in d])


def auc_without_zeros(data):
    """An AUCData without its zero-count entries: what psg_auc_merge keeps
    (include/psg.h, defined deviation)."""
    tk, tc, fk, fc = data
    return tk[tc != 0], tc[tc != 0], fk[fc != 0], fc[fc != 0]


def auc_data_digest(data):
    tk, tc, fk, fc = data
    return sha256([np.asarray(tk, np.int64), np.asarray(tc, np.uint64), np.asarray(fk, np.int64),
                   np.asarray(fc, np.uint64)])


class ExactCase:
    def __init__(self, name, y, p):
        self.name, self.y, self.p = name, y, p

    def digest(self):
        return sha256([fbits(self.y), fbits(self.p)])


def exact_auc_cases():
    """[ExactCase] whose result does not depend on how a sort orders equal
    predictions (the reference's std::sort leaves that open): all predictions
    distinct, negatives among them; or ties only among examples of one class
    (the class is a function of the prediction), -0.0 and +0.0 among them."""
    pos_l, neg_l = np.array([1.0, 0.5, 2.0]), np.array([-1.0, 0.0, -0.0, np.nan])
    out = []
    for i, n in enumerate(pin_sizes()):
        s = 53000 + 100 * i
        perm = np.argsort(splitmix64(s, n), kind="stable")
        out.append(ExactCase("distinct_n%d" % n, auc_labels(s + 1, n),
                             (perm - n // 2).astype(np.float64) * 0.5 + 0.25))
        v = (splitmix64(s + 2, n) % _u(37)).astype(np.int64) - 18
        d = splitmix64(s + 3, n)
        p = v.astype(np.float64) / 4.0
        p[(v == 0) & chance(d, 0.5)] = -0.0
        positive = ((v // 3) % 2 == 0)
        y = np.where(positive, pos_l[(d % _u(3)).astype(np.int64)], neg_l[(d % _u(4)).astype(np.int64)])
        out.append(ExactCase("ties_in_one_class_n%d" % n, y, p))
    return out


# ------------------------------------------------------------ localizer cases
# Inputs of localizer.npz (reference src/base/localizer.h over
# src/util/parallel_sort.h).  L40000 is past parallelSort's grain of 16,384
# pairs: with 4 threads the split into threads and std::inplace_merge run.
LOC_NAMES = ("L1", "Tm1", "T", "Tp1", "3Tp5", "L40000", "D40000")
LOC_THREADS = (1, 4)


def power_law(x, universe):
    """Draws as ranks in [0, universe), P(rank < r) = (r / universe)^(1/3), in
    integer arithmetic: rank 0 takes universe^(-1/3) of the draws."""
    r = x >> _u(32)
    q = (r * r) >> _u(32)
    q = (q * r) >> _u(32)
    return ((q * _u(universe)) >> _u(32)).astype(np.int64)


def csr_offsets(seed, n, rows):
    """rows + 1 offsets over n entries; with 5 rows or more the first, the
    middle and the last row are empty."""
    empty = {0, rows // 2, rows - 1} if rows >= 5 else set()
    live = [r for r in range(rows) if r not in empty]
    cuts = np.sort((splitmix64(seed, len(live) - 1) % _u(n + 1)).astype(np.int64))
    lens = np.zeros(rows, np.int64)
    lens[live] = np.diff(np.concatenate([[0], cuts, [n]]))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


class LocCase:
    def __init__(self, name, offset, index, value, dicts):
        self.name, self.offset, self.index, self.value, self.dicts = name, offset, index, value, dicts

    def digest(self):
        arrs = [self.offset, self.index] + ([] if self.value is None else [fbits(self.value)])
        for d in sorted(self.dicts):
            arrs.append(self.dicts[d])
        return sha256(arrs)


def loc_dicts(uniq, edges):
    """The dictionaries of a case whose ids are uniq (ascending).  edges:
    there is room below the smallest id and above the largest."""
    between = uniq[::2] + _u(1)
    between = between[~np.isin(between, uniq)]
    lo, hi = uniq[0], uniq[-1]
    absent = [between]
    d = {"all": uniq.copy(), "third": uniq[::3].copy(), "one": uniq[uniq.size // 2:uniq.size // 2 + 1].copy(),
         "empty": np.zeros(0, np.uint64)}
    if edges:
        below = np.array([lo - _u(900), lo - _u(2), lo - _u(1)], np.uint64)
        above = np.array([hi + _u(1), hi + _u(2), hi + _u(900)], np.uint64)
        d["below"], d["above"] = below, above  # matched = 0: a matrix of zero entries
        absent += [below, above]
    d["absent"] = np.unique(np.concatenate([uniq] + absent))
    return {k: np.ascontiguousarray(v) for k, v in d.items()}


def loc_case(name):
    """L1: one entry, one row.  Tm1 / T / Tp1 / 3Tp5: around the sort tile.
    L40000 / D40000: past parallelSort's grain, long runs / all distinct."""
    T = PIN_TILE
    n, kind, rows, binary = {"L1": (1, "one", 1, False), "Tm1": (T - 1, "zipf", 60, False),
                             "T": (T, "distinct", 41, True), "Tp1": (T + 1, "zipf", 1, True),
                             "3Tp5": (3 * T + 5, "edges", 200, False),
                             "L40000": (40000, "zipf", 1500, False),
                             "D40000": (40000, "distinct", 700, True)}[name]
    s = 54000 + 100 * LOC_NAMES.index(name)
    # ids that use the high digits (above 2^32, above 2^63), with room at both ends
    table = unique_keys(s, 3000 if kind != "distinct" else n)
    table = table[(table > _u(1 << 10)) & (table < _u(U64 - (1 << 10)))]
    if kind == "one":
        index = np.array([(1 << 63) + 12345], np.uint64)
    elif kind == "distinct":
        assert table.size >= n - 8
        index = np.concatenate([table, np.arange(5, 5 + n - table.size, dtype=np.uint64) << _u(33)])
        index = index[np.argsort(splitmix64(s + 1, n), kind="stable")]
    else:
        table = table[np.argsort(splitmix64(s + 2, table.size), kind="stable")]  # rank is not id order
        if kind == "edges":
            table[5], table[9] = 0, U64 - 1  # 0 and 2^64 - 2 among the frequent ids
        index = table[power_law(splitmix64(s + 1, n), table.size)]
    index = np.ascontiguousarray(index)
    assert index.size == n
    value = None if binary else scaled(splitmix64(s + 3, n), np.float64)
    if value is not None and n > 3:
        value[[0, 1, 2]] = [-0.0, 5e-324, np.nan]
    return LocCase(name, csr_offsets(s + 4, n, rows), index, value,
                   loc_dicts(np.unique(index), kind != "edges"))


def random_loc_case(seed):
    """Seeded cases beyond the fixtures (live tests)."""
    n = [1, 7, 300, 2049, 5000, 20000, 33000, 70000][seed % 8]
    rows = [1, 3, 10, 1, 77, 300, 2, 1000][seed % 8]
    s = 55000 + 100 * seed
    table = unique_keys(s, [1, 5, 40, 3000, 200, 19000, 9, 50000][seed % 8])
    table = table[(table > _u(1 << 10)) & (table < _u(U64 - (1 << 10)))]
    table = table[np.argsort(splitmix64(s + 2, table.size), kind="stable")]
    index = np.ascontiguousarray(table[power_law(splitmix64(s + 1, n), table.size)])
    value = None if seed % 2 else scaled(splitmix64(s + 3, n), np.float64)
    return LocCase("R%d" % seed, csr_offsets(s + 4, n, rows), index, value,
                   loc_dicts(np.unique(index), True))


def random_auc_case(seed):
    g = [1, 10, 100, 1000, 100000, -1000, 7, -3][seed % 8]
    n = [1, 2, 100, 2049, 5000, 333, 64, 4097][seed % 8]
    s = 56000 + 100 * seed
    p = _place(s + 2, spread20(splitmix64(s, n)), np.concatenate([auc_undefined(g), auc_specials(g)]))
    return AucCase("R%d" % seed, auc_labels(s + 1, n), p, g)


def record_output(arrays, sha, key, a):
    """Recorder only: every output's SHA-256, and the array itself when it is
    at most ARRAY_CAP bytes.  Doubles are passed as their bits."""
    a = np.ascontiguousarray(a)
    assert a.dtype.kind in "iub"
    sha[key] = sha256([a])
    if a.nbytes <= ARRAY_CAP:
        arrays[key] = a


def same_output(arrays, sha, key, got):
    """got (same dtype as recorded; doubles as their bits) against a recorded
    output: the array where the fixture holds it, and its SHA-256 always."""
    got = np.ascontiguousarray(got)
    if key in arrays:
        want = arrays[key]
        if want.dtype != got.dtype or want.shape != got.shape or not np.array_equal(want, got):
            return False
    return sha256([got]) == sha[key]


def remapped_from_tagged(n, new_index, new_value):
    """remapped_idx (localizer.h:123-136) is a local of remapIndex.  Run with
    value[j] = j, the returned matrix says which positions survived (new_value)
    and what each was mapped to (new_index): remapped_idx[j] = new_index[k] + 1
    for the k-th survivor j, and 0 for every dropped position."""
    r = np.zeros(n, np.uint32)
    r[np.asarray(new_value, np.float64).astype(np.int64)] = np.asarray(new_index, np.uint32) + np.uint32(1)
    return r


# --------------------------------------------------------------- snappy cases
# Inputs of tests/golden/snappy_pin/*.npz: tools/record_snappy.py compresses
# each with the real snappy compressor and stores the stream.  One fixture file
# per group.  The n of each case was chosen by search with the recorder
# (element = a literal or a copy after the preamble, what the table form of
# psg_snappy.hip counts against kTabMax = 4096); recorded with snappy 1.1.8:
#
#   case               n   bytes elements  copy-1 high-bit  longest   npend
#                                                           copy run
#   keys24          1000    8000     1997     997        0        1     971
#   keys40_le       2221   17768     4095    1988       23        1    1070
#   keys40_gt       2222   17776     4097    1988       22        1       -
#   keys_dense      8200   65600    16369    8150       73        2       -
#   keys63          2000   16000        1       0        0        0       0
#   f32_eighths     6000   24000     5755    5339     2095      503       -
#   f64_sent70      3000   24000     1559     292      138        3     897
#   f64_sent98      9000   72000     1424      34       16       33    1227
#   f64_sent_all    9000   72000     1127       0        0     1024    1117
#   f32_zero       20000   80000     1252       0        0     1024    1242
#   f32_gauss       1500    6000        1       0        0        0       0
#   abc             3000    9000      142       0        0      141     137
#   rep2047        6+12B   12294      149       1        1      148      21
#   rep2048        6+31B   12319      157       0        0      156      28
#   records          400   12800      749     370      349        1      17
#   alpha4          8000    8000     1909    1754     1016      208    1512
#   len0 .. len61: one literal each (none for len0)
# and the parts of the two pushes, pushA_p{0..3}_{keys,v0,v1} and
# pushB_p{0,1}_{keys,v0,v1} (their tallies are in the fixture's meta).
# keys40_le / keys40_gt: n draws are n keys here (no two collide); 2221 is the
# largest n in 2000..2499 with <= 4096 elements, 2222 the smallest with more
# (`tools/record_snappy.py --seam`).  high-bit: copy-1 elements whose offset is
# 256 or more, i.e. with a non-zero (tag >> 5) << 8 term.  npend: the copies
# the table form cannot place from the input (snappy_table_npend below, a host
# replay of the kernel's step 2); more than kTabPend = 64 of them, or more than
# kTabMax elements (-), and the streamed form decodes the part.  Key and value
# arrays are copies of copies, so all of them go that way; `records` (400
# records, chosen so that 1 <= npend <= 64 with hundreds of high-bit copy-1)
# is the stream the table form decodes itself.
SNAPPY_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snappy_pin")
SNAPPY_GROUPS = ("keys", "values", "bytes", "pushes")
SNAPPY_SEAM_N = (2221, 2222)  # keys below 2^40: <= 4096 elements, > 4096 elements
SNAPPY_EDGE_LENGTHS = (0, 1, 4, 15, 16, 17, 60, 61)
SENTINEL = U64  # Darling's inactive mark: every bit of the f64 set


class SnappyCase:
    def __init__(self, name, group, data):
        self.name, self.group, self.data = name, group, bytes(data)

    def digest(self):
        return hashlib.sha256(self.data).hexdigest()


def le_bytes(a):
    a = np.ascontiguousarray(a)
    return a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()


def random_bytes(seed, n):
    return le_bytes(splitmix64(seed, (n + 7) // 8))[:n]


def keys_below(seed, n, bits):
    """Sorted distinct keys below 2^bits out of n draws (nested in n)."""
    return np.unique(splitmix64(seed, n) >> _u(64 - bits))


def quantised(seed, n):
    """f32 multiples of 1/8 in [-4, 4)."""
    q = ((splitmix64(seed, n) >> _u(40)) % _u(64)).astype(np.int64) - 32
    return q.astype(np.float32) / np.float32(8)


def with_sentinel(seed, n, p):
    """f64 bits: scaled draws, the all-ones sentinel with probability p."""
    b = fbits(scaled(splitmix64(seed, n), np.float64)).copy()
    b[chance(splitmix64(seed + 1, n), p)] = _u(SENTINEL)
    return b


def near_gaussian(seed, n):
    """f32: the sum of twelve 20-bit uniforms, centred, / 2^20 (exact in f32;
    no libm, so the bits do not depend on the platform)."""
    x = splitmix64(seed, 12 * n).reshape(12, n) >> _u(44)
    return (x.sum(axis=0).astype(np.int64) - 6 * (1 << 20)).astype(np.float32) / np.float32(1 << 20)


def short_match_records(seed, n):
    """n records of 32 bytes: 24 fresh random bytes, then an 8-byte piece.
    From record 16 on the piece repeats 8 bytes of a record 8 to 55 back (256
    to 1,791 bytes): three times in four out of that record's fresh bytes,
    else that record's own piece.  The compressor turns each into a copy-1 of
    8 to 11 bytes whose source is literal data, or a copy one to a few levels
    above it: what the table form places straight from the input."""
    fresh = np.frombuffer(random_bytes(seed, 32 * n), np.uint8).reshape(n, 32).copy()
    draw = splitmix64(seed + 1, n)
    for r in range(16, n):
        d = int(draw[r])
        s = r - min(r, 8 + d % 48)
        a = 24 if (d >> 8) % 4 == 0 else (d >> 16) % 17
        fresh[r, 24:] = fresh[s, a:a + 8]
    return fresh.tobytes()


class SnappyPush:
    """A server key set D and value pushes [(keys, [vals] * m)], received as
    snappy parts.  `clean`: the pushes whose keys all lie in D."""

    def __init__(self, name, dtype, m, D, pushes, clean):
        self.name, self.dtype, self.m = name, np.dtype(dtype), m
        self.D, self.pushes, self.clean = D, pushes, clean

    def part_names(self, p):
        return ["push%s_p%d_keys" % (self.name, p)] + \
               ["push%s_p%d_v%d" % (self.name, p, i) for i in range(self.m)]


def snappy_push(name):
    if name == "A":
        # f32, m = 2: 3,000 server keys below 2^40, four pushes keeping each
        # with p = 0.4, values in eighths; the last push carries one key that
        # is not in D (the matched count falls one short of its size)
        D = keys_below(41000, 3000, 40)
        pushes = []
        for p in range(4):
            k = D[chance(splitmix64(41100 + p, D.size), 0.4)]
            if p == 3:
                extra = D[D.size // 2] + _u(1)
                assert not np.isin(extra, D)
                k = np.sort(np.append(k, extra))
            pushes.append((np.ascontiguousarray(k),
                           [quantised(41200 + 10 * p + i, k.size) for i in range(2)]))
        return SnappyPush(name, np.float32, 2, D, pushes, (0, 1, 2))
    if name == "B":
        # f64, m = 2, Darling's G (signed) and U (non-negative) of a block: 4,000
        # server keys, two pushes keeping each with p = 0.3; a key held by one
        # push alone is inactive (the sentinel, in both arrays) with p = 0.86,
        # about 60 % of a push -- never on a key both pushes hold, so that no
        # two NaNs meet in an add
        D = keys_below(42000, 4000, 40)
        keep = [chance(splitmix64(42100 + p, D.size), 0.3) for p in range(2)]
        pushes = []
        for p in range(2):
            k = D[keep[p]]
            off = (keep[p] & ~keep[1 - p])[keep[p]] & chance(splitmix64(42150 + p, k.size), 0.86)
            g = fbits(scaled(splitmix64(42200 + p, k.size), np.float64)).copy()
            u = fbits(np.abs(scaled(splitmix64(42300 + p, k.size), np.float64))).copy()
            g[off] = u[off] = _u(SENTINEL)
            pushes.append((np.ascontiguousarray(k), [g.view(np.float64), u.view(np.float64)]))
        return SnappyPush(name, np.float64, 2, D, pushes, (0, 1))
    raise KeyError(name)


SNAPPY_PUSH_NAMES = ("A", "B")


def snappy_cases():
    """[SnappyCase]: what the wire carries, as bytes."""
    out = []

    def add(group, name, data):
        out.append(SnappyCase(name, group, data if isinstance(data, bytes) else le_bytes(data)))
    # sorted distinct uint64 keys
    add("keys", "keys24", keys_below(40001, 1000, 24))
    add("keys", "keys40_le", keys_below(40002, SNAPPY_SEAM_N[0], 40))
    add("keys", "keys40_gt", keys_below(40002, SNAPPY_SEAM_N[1], 40))
    add("keys", "keys_dense", np.arange(8200, dtype=np.uint64) * _u(3) + _u(7))
    add("keys", "keys63", keys_below(40003, 2000, 63))
    # values
    add("values", "f32_eighths", quantised(40010, 6000))
    add("values", "f64_sent70", with_sentinel(40020, 3000, 0.70))
    add("values", "f64_sent98", with_sentinel(40030, 9000, 0.98))
    add("values", "f64_sent_all", np.full(9000, SENTINEL, np.uint64))
    add("values", "f32_zero", np.zeros(20000, np.float32))
    add("values", "f32_gauss", near_gaussian(40040, 1500))
    # byte patterns
    add("bytes", "abc", b"abc" * 3000)
    # a block six times and the first t bytes of a seventh: the compressor cuts
    # the one long match into 64-byte copies and a rest; t makes the rest 11
    # bytes, short enough for a copy-1 where the offset allows one (2047: the
    # largest, tag 0xfd) and a copy-2 where it does not (2048)
    for n, t in ((2047, 12), (2048, 31)):
        block = random_bytes(40050 + n, n)
        add("bytes", "rep%d" % n, block * 6 + block[:t])
    add("bytes", "records", short_match_records(40070, 400))
    add("bytes", "alpha4", bytes(b"acgt"[i] for i in (splitmix64(40052, 8000) >> _u(62)).tolist()))
    for n in SNAPPY_EDGE_LENGTHS:
        add("bytes", "len%d" % n, random_bytes(40060 + n, n))
    for pn in SNAPPY_PUSH_NAMES:
        c = snappy_push(pn)
        for p, (k, vs) in enumerate(c.pushes):
            for name, a in zip(c.part_names(p), [k] + [fbits(v) for v in vs]):
                add("pushes", name, a)
    return out


def snappy_elements(stream):
    """The tag walk of a raw snappy stream: (declared length, [(position of
    the tag, kind, length, offset-or-literal-header-bytes)]), kind 0 = literal,
    1 / 2 / 4 = copy with that many offset bytes.  Stops at the first element
    that does not fit the stream (a cut one is not listed)."""
    s, p, ulen, shift = bytes(stream), 0, 0, 0
    while True:
        if p >= len(s) or p >= 5:
            return None, []
        b = s[p]
        ulen |= (b & 0x7F) << shift
        shift += 7
        p += 1
        if not b & 0x80:
            break
    el = []
    while p < len(s):
        tag = s[p]
        kind = tag & 3
        if kind == 0:
            nb = max(tag >> 2, 59) - 59
            if p + 1 + nb > len(s):
                break
            ln = (int.from_bytes(s[p + 1:p + 1 + nb], "little") if nb else tag >> 2) + 1
            if p + 1 + nb + ln > len(s):
                break
            el.append((p, 0, ln, 1 + nb))
            p += 1 + nb + ln
        else:
            nb = (1, 2, 4)[kind - 1]
            if p + 1 + nb > len(s):
                break
            field = int.from_bytes(s[p + 1:p + 1 + nb], "little")
            if kind == 1:
                el.append((p, 1, 4 + (tag >> 2 & 7), (tag >> 5) << 8 | field))
            else:
                el.append((p, nb, (tag >> 2) + 1, field))
            p += 1 + nb
    return ulen, el


def snappy_tally(stream):
    """What a stream holds, for the fixtures' meta and the coverage asserts."""
    ulen, el = snappy_elements(stream)
    t = dict(uncompressed=ulen, elements=len(el), literals=0, lit_inline=0, lit_1byte=0, lit_2byte=0,
             lit_3byte=0, copy1=0, copy1_high=0, copy1_max_offset=0, copy2=0, copy2_min_offset=0,
             copy4=0, overlapping=0, longest_copy_run=0)
    run = 0
    for _, kind, ln, x in el:
        if kind == 0:
            t["literals"] += 1
            t[("lit_inline", "lit_1byte", "lit_2byte", "lit_3byte")[min(x - 1, 3)]] += 1
            run = 0
            continue
        run += 1
        t["longest_copy_run"] = max(t["longest_copy_run"], run)
        t["overlapping"] += x < ln
        if kind == 1:
            t["copy1"] += 1
            t["copy1_high"] += x >= 256
            t["copy1_max_offset"] = max(t["copy1_max_offset"], x)
        elif kind == 2:
            t["copy2"] += 1
            t["copy2_min_offset"] = min(t["copy2_min_offset"] or x, x)
        else:
            t["copy4"] += 1
    t = {k: int(v) for k, v in t.items()}
    t["table_npend"] = snappy_table_npend(el)
    return t


K_TAB_MAX, K_TAB_PEND, K_TAB_DEPTH = 4096, 64, 4  # psg_snappy.hip kTabMax, kTabPend, kTabDepth


def snappy_table_npend(el):
    """The table form's own count of the copies it cannot place from the input
    (psg_snappy.hip snappy_tab_kernel step 2, `resolve`): byte l of a copy at
    output position o with offset a repeats output byte o - a + l mod a; that
    byte is looked up in the element table, and if it lies in a copy, followed
    through that copy in the same way, kTabDepth look-ups at the most.  A copy
    with a byte that has not reached a literal by then is left for step 3, and
    a part with more than kTabPend of them is decoded again by the streamed
    form.  None for a part of more than kTabMax elements (the walk stops
    there and the streamed form decodes it)."""
    if len(el) > K_TAB_MAX:
        return None
    if not el:
        return 0
    kind = np.array([e[1] for e in el], np.int64)
    ln = np.array([e[2] for e in el], np.int64)
    off = np.where(kind > 0, np.array([e[3] for e in el], np.int64), 1)
    x = np.concatenate([[0], np.cumsum(ln)[:-1]])  # output position of each element
    copies = np.nonzero(kind > 0)[0]
    if copies.size == 0:
        return 0
    owner = np.repeat(copies, ln[copies])  # one entry per copied byte
    l = np.arange(owner.size) - np.repeat(np.cumsum(ln[copies]) - ln[copies], ln[copies])
    q = x[owner] - off[owner] + l % off[owner]
    open_ = np.ones(owner.size, bool)
    for _ in range(K_TAB_DEPTH):
        j = np.searchsorted(x, q, "right") - 1
        lit = kind[j] == 0
        open_ &= ~lit
        q = np.where(lit, q, x[j] - off[j] + (q - x[j]) % off[j])
    return int(np.unique(owner[open_]).size)


def snappy_form(tally):
    """Which decoder a part of a launch of <= 64 parts ends in."""
    n = tally["table_npend"]
    return "table" if n is not None and n <= K_TAB_PEND else "streamed"


_recorded = {}


def snappy_recorded():
    """{name: (case, recorded stream, recorded info)} in case order, each
    input's SHA-256 checked against the fixture; built once, read only."""
    if not _recorded:
        fx = {g: load_fixture(g, SNAPPY_GOLDEN) for g in SNAPPY_GROUPS}
        for c in snappy_cases():
            meta, arrays = fx[c.group]
            info = meta["cases"][c.name]
            assert info["input_sha256"] == c.digest(), c.name
            _recorded[c.name] = (c, arrays[c.name].tobytes(), info)
        assert sum(len(m["cases"]) for m, _ in fx.values()) == len(_recorded)
    return _recorded


def snappy_truncations(stream):
    """[(what, bytes)]: a stream cut after its preamble, in a copy-1 (tag
    present, offset byte missing), in a literal and one byte short."""
    ulen, el = snappy_elements(stream)
    copy1 = [e for e in el if e[1] == 1]
    lit = [e for e in el if e[1] == 0 and e[2] >= 2 and e[0] > el[0][0]]
    c, lt = copy1[len(copy1) // 2], lit[len(lit) // 2]
    return [("preamble", stream[:el[0][0]]), ("copy1", stream[:c[0] + 1]),
            ("literal", stream[:lt[0] + lt[3] + lt[2] // 2]), ("short", stream[:-1])]


# -------------------------------------------------------------------- fixtures
def save_fixture(name, meta, arrays, directory=GOLDEN):
    """Recorder only.  meta: JSON-able; arrays: little-endian numpy arrays."""
    os.makedirs(directory, exist_ok=True)
    blob = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    np.savez_compressed(os.path.join(directory, name + ".npz"), meta=blob, **arrays)


def load_fixture(name, directory=GOLDEN):
    with np.load(os.path.join(directory, name + ".npz")) as z:
        arrays = {k: z[k] for k in z.files if k != "meta"}
        meta = json.loads(z["meta"].tobytes().decode())
    return meta, arrays
