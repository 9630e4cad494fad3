"""TEST INFRASTRUCTURE: a plain-integer model of the N-way merge's planning
stages (parameter_server_amd/csrc/psg_nway.hip, stages 0-4) and the inputs
of its edge tests.

What is modelled, per merge: the shape (NwShape::plan), the candidates (every
s-th key of every push), the rank estimate A(c) = s * sum_q lower_bound(
candidates of push q, c), the buckets floor(A / cw) with their largest
candidate, the prefix max (the splitters), the seg table (lower_bound of
every push at every splitter) and from it the piece and tile sizes.  For a
batch: the rank kernel's form and the ticket order (NwPlan::plan_shapes).
The tile kernel itself (stage 5) is not modelled: the tests compare its
output with oracle_py.

Two searches.  `exact` (numpy searchsorted) is lower_bound of a sorted
array.  `device` is a literal transcription of dev::interp_lower_bound /
dev::bracket_lower_bound (psg_device.h) in Python integers, the u64 wrap of
`xl - ka` and the saturating double -> u64 conversion included: on a
disordered array it returns what the kernels' search returns, which is not
a lower bound of anything.  The model of a disordered merge is that of rank
form 1 (one merge, or a small batch), whose rank stage searches the
candidate lists with the same function; the LDS searches of forms 16 and 4
are only modelled for sorted lists, where every correct search agrees.

For a disordered merge the model's `distinct` of a tile (its number of
different keys) is a LOWER bound of what the tile kernel stores (it stores
one entry per key that differs from its predecessor in the merged, then
unsorted, sequence), and a tile's size is an UPPER bound.

Inputs come from pin_cases.splitmix64, never from a library generator.
"""
import numpy as np

from pin_cases import splitmix64

M64 = (1 << 64) - 1
CAP = 2048        # kNwCap: elements per tile
PER = 8           # kNwPer: outputs per thread
MAX_RUNS = 64     # kNwMaxRuns
RK_LIST = 8192    # kRkList: candidates of one list staged in LDS
_u = np.uint64


# ---------------------------------------------------------------- the plan
def shape(ns):
    """NwShape::plan over the non-empty pushes of lengths ns."""
    ns = [int(n) for n in ns if int(n) != 0]
    K = len(ns)
    s = max(1, CAP // (8 * max(K, 1)))
    cw = CAP - 2 * K * s
    cbase = [0]
    for n in ns:
        cbase.append(cbase[-1] + n // s)
    B = sum(ns) // cw + 1
    T = B + 1
    if K == 0:
        B = T = 0
    return dict(K=K, s=s, cw=cw, B=B, T=T, ncand=cbase[-1], cbase=cbase, ns=ns, ntot=sum(ns))


def _waves(ncand, per):
    return (ncand + 256 * per - 1) // (256 * per)


def batch_plan(merges_ns):
    """NwPlan::plan_shapes: (shapes, rank form, round robin, tickets)."""
    sh = [shape(ns) for ns in merges_ns]
    w16 = sum(_waves(x["ncand"], 16) for x in sh)
    w4 = sum(_waves(x["ncand"], 4) for x in sh)
    form = 16 if w16 >= 512 else (4 if w4 >= 512 else 1)
    ntiles = sum(x["T"] for x in sh)
    maxT = max([x["T"] for x in sh] + [0])
    nm = len(sh)
    rr = nm > 1 and maxT * nm <= 2 * ntiles
    return sh, form, rr, (maxT * nm if rr else ntiles)


# ------------------------------------------------------------- the searches
def _f2u64(x):
    """(uint64_t)double as the device converts: NaN and negatives 0, values
    from 2^64 up saturate."""
    if x != x or x <= 0.0:
        return 0
    if x >= 18446744073709551616.0:
        return M64
    return int(x)


def _div(a, b):
    if b == 0.0:
        return float("nan") if a == 0.0 else float("inf")
    return a / b


def bracket_lower_bound(S, xl, a, c, ka, kc):
    """dev::bracket_lower_bound, line by line.  S: a list of Python ints.  An
    index outside S raises IndexError (the device would read out of bounds)."""
    def at(i):
        if not 0 <= i < len(S):
            raise IndexError("bracket_lower_bound reads S[%d] of %d" % (i, len(S)))
        return S[i]
    it = 0
    while it < 6 and ((c - a) & M64) > 16:
        f = _div(float((xl - ka) & M64), float((kc - ka) & M64))
        mid = (a + 1 + _f2u64(f * float((c - a - 1) & M64))) & M64
        mid = mid if mid < c else (c - 1) & M64
        km = at(mid)
        if km < xl:
            a, ka = mid, km
        else:
            c, kc = mid, km
        it += 1
    while ((c - a) & M64) > 16:
        mid = (a + (((c - a) & M64) >> 1)) & M64
        if at(mid) < xl:
            a = mid
        else:
            c = mid
    below = 0
    for i in range(1, 16):
        idx = a + i if a + i < c else c
        below += 1 if at(idx) < xl else 0
    return a + 1 + below


def interp_lower_bound(S, x):
    """dev::interp_lower_bound: in [0, n] whatever S holds."""
    n = len(S)
    if n == 0:
        return 0
    k0, kn = S[0], S[n - 1]
    if x <= k0:
        return 0
    if x > kn:
        return n
    return bracket_lower_bound(S, x, 0, n - 1, k0, kn)


# --------------------------------------------------------------- one merge
class Merge:
    """Stages 0-4 of one merge of `pushes` (uint64 arrays; empty ones are
    dropped as nway_create drops them).  device=False: exact lower bounds
    (sorted pushes only); device=True: the kernels' search, transcribed."""

    def __init__(self, pushes, device=False):
        self.pushes = [np.ascontiguousarray(p, np.uint64) for p in pushes if len(p)]
        sh = self.shape = shape([p.size for p in self.pushes])
        K, s, cw, B, T = (sh[k] for k in ("K", "s", "cw", "B", "T"))
        cands = [p[s - 1::s][: p.size // s] for p in self.pushes]
        ckeys = np.concatenate(cands) if K else np.zeros(0, np.uint64)
        if device:
            lists = [p.tolist() for p in self.pushes]
            clists = [c.tolist() for c in cands]
            lb_c = lambda q, keys: np.array([interp_lower_bound(clists[q], k) for k in keys.tolist()], np.int64)  # noqa: E731
            lb_p = lambda q, keys: [interp_lower_bound(lists[q], k) for k in keys]  # noqa: E731
        else:
            lb_c = lambda q, keys: np.searchsorted(cands[q], keys, "left").astype(np.int64)  # noqa: E731
            lb_p = lambda q, keys: np.searchsorted(self.pushes[q], np.array(keys, np.uint64), "left").tolist()  # noqa: E731
        # 0 / 1: candidates and A(c)
        rank = np.zeros(ckeys.size, np.int64)
        for q in range(K):
            rank += lb_c(q, ckeys)
        rank *= s
        self.cand_keys = ckeys.tolist()
        self.rank = rank.tolist()
        # 2 / 3: buckets, prefix max
        split = np.zeros(B, np.uint64)
        inb = rank // cw < B
        np.maximum.at(split, rank[inb] // cw, ckeys[inb])
        split = np.maximum.accumulate(split) if B else split
        self.split = split = [int(x) for x in split.tolist()]
        # 4: seg[t][q]
        seg = [[0] * K]
        mids = [lb_p(q, split[: T - 1]) for q in range(K)] if T > 1 else []
        for t in range(1, T):
            seg.append([mids[q][t - 1] for q in range(K)])
        if T:
            seg.append([int(p.size) for p in self.pushes])
        self.seg = seg
        self.piece = [[max(0, seg[t + 1][q] - seg[t][q]) for q in range(K)] for t in range(T)]
        self.tile_sizes = [sum(x) for x in self.piece]

    @property
    def ntot(self):
        return self.shape["ntot"]

    def overflows(self):
        return [t for t, e in enumerate(self.tile_sizes) if e > CAP]

    def kept_elements(self):
        """Elements of the tiles that do not overflow (an overflowing tile is
        merged as empty): an upper bound of the entries the run stores."""
        return sum(e for e in self.tile_sizes if e <= CAP)

    def distinct(self):
        """Different keys per non-overflowing tile, summed: a lower bound of
        the entries the run stores."""
        tot = 0
        for t, e in enumerate(self.tile_sizes):
            if e > CAP:
                continue
            ks = [self.pushes[q][self.seg[t][q]: self.seg[t][q] + self.piece[t][q]]
                  for q in range(self.shape["K"])]
            tot += np.unique(np.concatenate(ks)).size if ks else 0
        return tot

    def locate(self, key):
        """(tile, offset): the tile holding `key` and the merged position in
        it of the key's first copy (sorted pushes)."""
        key = int(key)
        T = self.shape["T"]
        t = next(t for t in range(T) if t + 1 >= T or key < self.split[t])
        below = sum(int(np.searchsorted(p, _u(key), "left")) - self.seg[t][q]
                    for q, p in enumerate(self.pushes))
        return t, below


# ---------------------------------------------------------------- inputs
def draws(seed, n):
    return splitmix64(seed, n)


def sorted_keys(seed, n, bits=64):
    """n distinct sorted keys below 2^bits."""
    k = np.unique(splitmix64(seed, n + n // 4 + 64) >> _u(64 - bits))
    assert k.size >= n
    pick = np.sort(np.argsort(splitmix64(seed + 1, k.size), kind="stable")[:n])
    return np.ascontiguousarray(k[pick])


def lengths(seed, count, lo, hi):
    """count lengths in [lo, hi]."""
    return (lo + (splitmix64(seed, count) % _u(hi - lo + 1)).astype(np.int64)).tolist()


def form16_lengths(nm=512):
    """nm merges of K = 3 ragged pushes of 200-600 keys: at least one
    candidate and so one rank workgroup each (rank form 16 from 512 up)."""
    ns = lengths(1200, 3 * nm, 200, 600)
    return [ns[3 * j: 3 * j + 3] for j in range(nm)]


def values(seed, n, dtype):
    """Signed finite values: integers scaled by a power of two, so sums of a
    few need more bits than the format has and the fold order shows."""
    x = splitmix64(seed, n)
    if np.dtype(dtype) == np.float32:
        return ((x >> _u(40)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 12)
    return ((x >> _u(11)).astype(np.int64) - (1 << 52)).astype(np.float64) / np.float64(1 << 40)


SORTED_2500 = np.arange(2500, dtype=np.uint64) * _u(7)


def case_a():
    """A sorted push beside 6,000 copies of one key."""
    return [SORTED_2500, np.full(6000, 5, np.uint64)]


def case_b():
    """A sorted push beside a rotated sorted push."""
    return [SORTED_2500, np.roll(np.arange(6000, dtype=np.uint64) * _u(3), 2000)]


def case_reversed():
    return [SORTED_2500, (np.arange(6000, dtype=np.uint64) * _u(3))[::-1].copy()]


def case_dup_run():
    """A sorted push whose middle holds a run of 400 equal keys."""
    k = np.arange(6000, dtype=np.uint64) * _u(3)
    k[3000:3400] = k[3000]
    return [SORTED_2500, k]


def cubed_keys(seed, n):
    """Up to n distinct sorted keys below 2^16, dense near 0: u^3 / 2^32 of
    16-bit draws u (integer arithmetic).  An interpolation search of such
    keys probes far from where the key is, so on a disordered push its
    probes reach the displaced blocks."""
    u = splitmix64(seed, 4 * n + 64) >> _u(48)
    k = np.unique((u * u * u) >> _u(32))
    pick = np.sort(np.argsort(splitmix64(seed + 1, k.size), kind="stable")[:n])
    return np.ascontiguousarray(k[pick])


# case_c seeds, found by search_case_c over range(40000): the first whose
# merge overflows a tile, and the first that over-produces (the tiles that do
# not overflow hold more different keys than sum(n): 258 more)
CASE_C_OVERFLOW_SEED = 28
CASE_C_OVERPRODUCE_SEED = 3229


def case_c(seed):
    """K = 2, keys below 2^16 (cubed_keys): a sorted push of 2,500-4,999 keys
    and a push of 900-2,399 keys with two blocks of 2-121 keys exchanged."""
    r = splitmix64(seed, 8)
    na, nb = 2500 + int(r[0] % _u(2500)), 900 + int(r[1] % _u(1500))
    a, b = cubed_keys(seed * 4 + 1, na), cubed_keys(seed * 4 + 2, nb)
    nb = b.size
    l1, l2 = 2 + int(r[2] % _u(120)), 2 + int(r[3] % _u(120))
    p1 = int(r[4] % _u(nb - l1 - l2 - 1))
    p2 = p1 + l1 + int(r[5] % _u(nb - p1 - l1 - l2))
    moved = np.concatenate([b[:p1], b[p2:p2 + l2], b[p1 + l1:p2], b[p1:p1 + l1], b[p2 + l2:]])
    assert moved.size == nb
    return [a, moved]


def search_case_c(want, seeds=range(3000)):
    """The first seeded case C for which want(Merge) holds: (seed, pushes)."""
    for seed in seeds:
        pushes = case_c(seed)
        if want(Merge(pushes, device=True)):
            return seed, pushes
    return None, None
