"""TEST INFRASTRUCTURE: the fixed inputs of the reference-pinning fixtures
(tests/golden/reference_pin/*.npz) and their loader.

tools/record_reference.py runs the reference's own code (oracle/_ref, built
from the reference tree by oracle/Makefile) on these inputs and stores what
it returns; tests/test_reference_pin.py (CPU) and the GPU tests rebuild the
same inputs here, check their SHA-256 against the fixture and compare bit for
bit.  Every input comes from splitmix64 in numpy uint64 arithmetic, never
from a library RNG, so a fixture does not depend on the numpy version.
Floats are integers scaled by a power of two, plus listed special values.

What the inputs avoid, and why: two NaNs never meet in one add (which
payload survives is not fixed by IEEE 754) and +inf never meets -inf, nor
0 an infinity in a product (the default NaN's sign differs between x86 and
the GPU).  Everything else -- -0.0, single NaNs quiet and signalling, +-inf,
denormals, 0xFFFFFFFF counts -- is in.
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


# -------------------------------------------------------------------- fixtures
def save_fixture(name, meta, arrays):
    """Recorder only.  meta: JSON-able; arrays: little-endian numpy arrays."""
    os.makedirs(GOLDEN, exist_ok=True)
    blob = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), meta=blob, **arrays)


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        arrays = {k: z[k] for k in z.files if k != "meta"}
        meta = json.loads(z["meta"].tobytes().decode())
    return meta, arrays
