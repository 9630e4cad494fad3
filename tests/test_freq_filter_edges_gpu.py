"""The count-min filter's kernels (psg_countmin.hip) at their block, region,
wave and tile edges.  tests/test_freq_filter.py compares the filter with the
oracle at workload-shaped sizes; here the shapes are chosen from the kernels'
tile constants, restated below.

Everything is exact: table bytes with np.array_equal on psg_freq_table, kept
keys in input order, against oracle/psg_oracle.c (orc_cm_*, pinned to the
reference's recorded tables by tests/test_reference_pin.py).  Query tables
are uniform random bytes set with psg_freq_table_assign, so the query cases
do not depend on insert; one case queries a table built by inserts.

The CPU tests at the end run the oracle alone: they check that the case
lists really hold the shapes they are meant to (blocks per wave and trip,
a full block of records, both sides of the query form switch) and that each
query case's thresholds keep a real fraction of its keys.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_py as O

# ---- the kernels' constants (parameter_server_amd/csrc/psg_countmin.hip) ----
INS_REGION = 32768       # kRegBytes: table bytes per insert region
INS_BLOCK_RECS = 32768   # kBlkRecs: records per insert block; a u16 region start reaches it
APPLY_WAVE_BLOCKS = 64   # cm_iapply_kernel: blocks a wave takes per trip
APPLY_WAVES = 16         # kBlkNT / 64
APPLY_TRIP = APPLY_WAVES * APPLY_WAVE_BLOCKS  # blocks per trip of the b0 loop
TRANSPOSE_TILE = 64      # cm_transpose_kernel: 64 x 64 tiles of (block, region column)
Q_REGION = 131072        # kQRegBytes: table bytes per query region
Q_MAX_REGIONS = 1024     # kQMaxReg
Q_MAX_K = 8              # kQMaxK
Q_TILE = 2048            # kQTile: keys per compaction tile
Q_LINE = 64              # bytes a direct probe is charged (launch_cm_query)


def ins_block_keys(k):   # ins_block_keys()
    return 8192 if k <= 4 else 4096 if k <= 8 else 2048 if k <= 16 else 1024


def q_block_keys(k):     # q_block_keys(): 13-bit key index in a result
    return 8192 if k <= 4 else 4096


def table_bytes(n):      # cm_table_bytes()
    return (n + 3) & ~3


def ins_regions(n):
    return (table_bytes(n) + INS_REGION - 1) // INS_REGION


def q_regions(n):
    return (table_bytes(n) + Q_REGION - 1) // Q_REGION


def q_is_binned(n, k, nk):
    """launch_cm_query's choice: the binned form when the direct form's probe
    lines would exceed the table."""
    return k <= Q_MAX_K and q_regions(n) <= Q_MAX_REGIONS and nk * k * Q_LINE > table_bytes(n)


def rand_keys(rng, nk):
    return rng.integers(0, 1 << 62, nk, dtype=np.uint64)


# ------------------------------------------------------------ insert cases --
# every case: (n, k, [(keys, counts), ...] one pair per psg_freq_insert call)
N3 = 3 * INS_REGION + 5   # four regions, the last 8 bytes
N2 = 2 * INS_REGION + 1   # three regions, the last 4 bytes

KEY_COUNT_EDGES = [1, 8191, 8192, 8193]                       # case 1 (k = 4, n = N3)
K_SWITCHES = [(5, 2 * 4096 + 1), (8, 2 * 4096 + 1), (9, 2 * 2048 + 1), (16, 2 * 2048 + 1),
              (17, 2 * 1024 + 1), (30, 2 * 1024 + 1), (4, 8192)]  # case 2 (k, nk), n = N2
APPLY_BLOCKS = [63, 64, 65, 1023, 1024, 1025, 1100]           # case 3 (k = 17, n = N3)
TRANSPOSE = [(r, nb) for r in (63, 64, 65) for nb in (64, 65)]  # case 4 (k = 4)
TABLE_SIZES = [64, 65, 67, 32767, 32768, 32769, 65536]        # case 6 (k = 3, nk = 3000)
WRAP_COUNTS = np.array([0, 1, 255, 256, 257, (1 << 32) - 1], np.uint32)


def case_key_count(nk):
    rng = np.random.default_rng(1000 + nk)
    return N3, 4, [(rand_keys(rng, nk), rng.integers(0, 700, nk).astype(np.uint32))]


def case_k_switch(k, nk):
    """Every count nonzero mod 2^8, so a full block holds KB * k records."""
    rng = np.random.default_rng(2000 + k)
    counts = (rng.integers(1, 256, nk) + 256 * rng.integers(0, 3, nk)).astype(np.uint32)
    return N2, k, [(rand_keys(rng, nk), counts)]


def case_apply_blocks(nb):
    rng = np.random.default_rng(3000 + nb)
    nk = 1024 * (nb - 1) + 1
    return N3, 17, [(rand_keys(rng, nk), rng.integers(0, 700, nk).astype(np.uint32))]


def case_transpose(r, nb):
    rng = np.random.default_rng(4000 + 100 * r + nb)
    nk = 8192 * (nb - 1) + 1
    return INS_REGION * r - 3, 4, [(rand_keys(rng, nk), rng.integers(0, 700, nk).astype(np.uint32))]


def case_repeats():
    """Call 1: one key 8192 times with count 255 (a whole block, 32768 records
    in four runs), the same key again in the second and the third block among
    random keys.  Call 2: every third key of 20,000 equal.  Counts from
    WRAP_COUNTS (byte wrap, and 0 / 256 whose records are dropped).
    8192 equal counts sum to 0 mod 2^8 whatever the count, so call 1's full
    block leaves its counters as they were; call 3 repeats another key 8192
    times with counts in [1, 256) whose sum is not 0 mod 2^8 (asserted by the
    CPU test below), then 100 random keys."""
    rng = np.random.default_rng(5000)
    x, y = np.uint64(0x1234567890ABCDEF >> 2), np.uint64(777)
    k1 = np.concatenate([np.full(8192, x, np.uint64), rand_keys(rng, 8192 + 777)])
    c1 = np.concatenate([np.full(8192, 255, np.uint32), rng.choice(WRAP_COUNTS, 8192 + 777)])
    for at in (8192 + 5, 2 * 8192 + 100):
        k1[at], c1[at] = x, 257
    k2 = rand_keys(rng, 20_000)
    k2[::3] = y
    c2 = rng.choice(WRAP_COUNTS, k2.size)
    k3 = np.concatenate([np.full(8192, np.uint64(31337), np.uint64), rand_keys(rng, 100)])
    c3 = rng.integers(1, 256, k3.size).astype(np.uint32)
    return N2, 4, [(k1, c1), (k2, c2), (k3, c3)]


def case_table_size(n):
    rng = np.random.default_rng(6000 + n)
    return n, 3, [(rand_keys(rng, 3000), rng.integers(0, 700, 3000).astype(np.uint32))]


def insert_shapes():
    """(n, k, nk) of every binned insert call above, without building the keys
    of the large ones."""
    out = [(N3, 4, nk) for nk in KEY_COUNT_EDGES]
    out += [(N2, k, nk) for k, nk in K_SWITCHES]
    out += [(N3, 17, 1024 * (nb - 1) + 1) for nb in APPLY_BLOCKS]
    out += [(INS_REGION * r - 3, 4, 8192 * (nb - 1) + 1) for r, nb in TRANSPOSE]
    out += [(N2, 4, keys.size) for keys, _ in case_repeats()[2]]
    out += [(n, 3, 3000) for n in TABLE_SIZES]
    return out


# ------------------------------------------------------------- query cases --
class QCase:
    def __init__(self, tag, n, k, nk, keys="random", dev=False):
        self.tag, self.n, self.k, self.nk, self.keys, self.dev = tag, n, k, nk, keys, dev

    def __repr__(self):
        return self.tag


# The issue's thresholds are (-1, 0, 40, 200, 254).  With uniform table bytes
# a key is kept with probability ((255 - f) / 256)^k: at k = 1 both 40 (84 %)
# and 200 (21 %) keep a real fraction, at larger k only thresholds nearer 0
# do, so the two middle ones move with k (k = 4: 40 -> 50 %, 90 -> 17 %;
# k = 8: 10 -> 70 %, 40 -> 25 %; k = 30: 3 -> 62 %, 10 -> 27 %).  -1 (keeps
# all), 0 and 254 stay in every list.
def default_freqs(k):
    mid = (40, 200) if k == 1 else (40, 90) if k <= 5 else (10, 40) if k <= 9 else (3, 10)
    return (-1, 0) + mid + (254,)


QN = 2 * Q_REGION + 3    # three query regions, the last 4 bytes
QBIG = 3_000_017         # 23 query regions
TILE_EDGES = [2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 8192 + 2049]
SWITCH_NK = [1, 100, 2049, 11_718, 11_719, 12_289]

Q_CASES = (
    # 1. compaction-tile and key-block edges
    [QCase("edge-k%d-nk%d" % (k, nk), QN, k, nk, dev=True) for k in (1, 4, 5, 8) for nk in TILE_EDGES]
    # 2. both sides of the form switch (k = 4: binned from 11,719 keys on)
    + [QCase("switch-nk%d" % nk, QBIG, 4, nk, dev=True) for nk in SWITCH_NK]
    # 3. k > 8: direct whatever the key count
    + [QCase("bigk-k%d" % k, QBIG, k, 20_001) for k in (9, 30)]
    # 4. long runs (8192 keys x 4 probes = 32768 records of a block in one
    # region) and region-count edges
    + [QCase("run-equal", QN, 4, 8193, keys="equal")]
    + [QCase("run-n%d" % n, n, 4, 8193) for n in (Q_REGION - 1, Q_REGION, Q_REGION + 1, Q_REGION + 64,
                                                  2 * Q_REGION - 1, 2 * Q_REGION + 1)]
)
Q_BY_TAG = {c.tag: c for c in Q_CASES}


@functools.lru_cache(maxsize=None)
def q_table(n, k):
    """Uniform random bytes; one table per (n, k), shared by the cases on it."""
    return np.random.default_rng(7000 + 31 * n + k).integers(0, 256, n, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def q_keys(tag):
    c = Q_BY_TAG[tag]
    rng = np.random.default_rng(8000 + c.nk + 97 * c.k + c.n % 1009)
    if c.keys == "equal":
        return np.full(c.nk, rand_keys(rng, 1)[0], np.uint64)
    return rand_keys(rng, c.nk)


@functools.lru_cache(maxsize=None)
def q_freqs(tag):
    """A case's thresholds.  A case with one distinct key (a single key, or
    all keys equal) keeps all of its keys or none, so its two middle
    thresholds sit at the key's own minimum m: m - 1 keeps it, m drops it."""
    c = Q_BY_TAG[tag]
    keys = q_keys(tag)
    if np.unique(keys).size > 1:
        return default_freqs(c.k)
    t, one = q_table(c.n, c.k), keys[:1]
    m = min(f for f in range(0, 255) if O.ff_query(t, c.n, c.k, one, f).size == 0)
    return tuple(sorted({-1, 0, m - 1, m, 254}))


@functools.lru_cache(maxsize=None)
def q_expect(tag):
    """{threshold: kept keys} from the oracle, computed once per case."""
    c = Q_BY_TAG[tag]
    t, keys = q_table(c.n, c.k), q_keys(tag)
    return {f: O.ff_query(t, c.n, c.k, keys, f) for f in q_freqs(tag)}


@functools.lru_cache(maxsize=None)
def insert_then_query_case():
    """Query case 6: k = 5, three query regions, 12,289 keys with repeats
    (every fifth key one of 16) inserted, then the same keys queried."""
    rng = np.random.default_rng(9000)
    keys = rand_keys(rng, 12_289)
    keys[::5] = keys[rng.integers(0, 16, keys[::5].size)]
    counts = rng.integers(0, 300, keys.size).astype(np.uint32)
    t, n, k = O.cm_resize(QN, 5)
    O.cm_insert(t, n, k, keys, counts)
    freqs = (-1, 0, 40, 200, 254)
    return keys, counts, t, {f: O.ff_query(t, n, k, keys, f) for f in freqs}


# ------------------------------------------------------------------ GPU --
def _ctx():
    import torch
    assert torch.cuda.is_available()
    from parameter_server_amd.kv_vector import KVVector
    return KVVector(0)


def _table(v, ch, n):
    from parameter_server_amd import _lib
    out = np.empty(n, np.uint8)
    _lib.check(v._L.psg_freq_table(v._h, ch, out.ctypes.data, n))
    return out


def _query(v, ch, keys, freq):
    from parameter_server_amd import _lib
    keys = np.ascontiguousarray(keys, np.uint64)
    out = np.empty(max(1, keys.size), np.uint64)
    m = C.c_size_t()
    _lib.check(v._L.psg_freq_query(v._h, ch, keys.ctypes.data, keys.size, freq, out.ctypes.data,
                                   C.byref(m)))
    return out[: m.value]


def _insert_case(case, ch=0):
    """Resize a fresh filter, make the case's insert calls, compare the table
    with the oracle's after each call."""
    from parameter_server_amd import _lib
    n, k, calls = case
    v = _ctx()
    _lib.check(v._L.psg_freq_resize(v._h, ch, n, k))
    t, nn, kk = O.cm_resize(n, k)
    assert (nn, kk) == (n, k)
    for i, (keys, counts) in enumerate(calls):
        _lib.check(v._L.psg_freq_insert(v._h, ch, keys.ctypes.data, counts.ctypes.data, keys.size))
        O.cm_insert(t, nn, kk, keys, counts)
        got = _table(v, ch, nn)
        bad = np.flatnonzero(got != t)
        assert bad.size == 0, "call %d: %d of %d counters differ, first at %d" % (
            i, bad.size, nn, bad[0])
        assert np.array_equal(got, t)
    assert t.any()
    v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nk", KEY_COUNT_EDGES)
def test_gpu_insert_key_count_edges(nk):
    """Insert case 1: one key, and a block of 8192 keys less one, exact, plus one."""
    _insert_case(case_key_count(nk))


@pytest.mark.gpu
@pytest.mark.parametrize("k,nk", K_SWITCHES)
def test_gpu_insert_k_at_block_size_switches(k, nk):
    """Insert case 2: two full blocks and one key, k on either side of each
    block-size switch, three regions; at k = 4, 8, 16 a full block's region
    starts end at exactly 32768."""
    _insert_case(case_k_switch(k, nk))


@pytest.mark.gpu
@pytest.mark.parametrize("nb", APPLY_BLOCKS)
def test_gpu_insert_apply_waves_and_trips(nb):
    """Insert case 3: the apply pass with a wave's 64 blocks less one, exact,
    plus one (a second wave), and a trip's 1024 blocks less one, exact, plus
    one and plus 76 (a second trip of waves 0 and 1)."""
    _insert_case(case_apply_blocks(nb))


@pytest.mark.gpu
@pytest.mark.parametrize("r,nb", TRANSPOSE)
def test_gpu_insert_transpose_tile_edges(r, nb):
    """Insert case 4: region-start columns 64, 65, 66 by 64 and 65 blocks."""
    _insert_case(case_transpose(r, nb))


@pytest.mark.gpu
def test_gpu_insert_repeats_and_byte_wrap():
    """Insert case 5 (case_repeats)."""
    _insert_case(case_repeats())


@pytest.mark.gpu
@pytest.mark.parametrize("n", TABLE_SIZES)
def test_gpu_insert_table_sizes(n):
    """Insert case 6: the minimum table, n % 4 != 0, a region less one,
    exact, plus one, and two exact regions."""
    _insert_case(case_table_size(n))


@pytest.mark.gpu
@pytest.mark.parametrize("check_each", [False, True])
def test_gpu_insert_scratch_across_calls_and_resize(check_each):
    """Insert case 7: one filter, inserts of 1, 70,001, 9 and 70,001 keys on a
    side stream (the record scratch grows, then is reused by smaller and equal
    inserts), then psg_freq_resize to the same n with k 4 -> 17 -> 2 (the table
    and the scratch stay, the table is cleared) and an insert after each.
    With check_each the table is compared after every insert; without, no
    host wait separates the calls of a k and the table is compared once
    before each resize and at the end."""
    import torch
    from parameter_server_amd import _lib
    rng = np.random.default_rng(7)
    n, ch = N3, 3
    plan = [(4, (1, 70_001, 9, 70_001)), (17, (70_001,)), (2, (30_001,))]
    host = [[(rand_keys(rng, nk), rng.integers(0, 700, nk).astype(np.uint32)) for nk in nks]
            for _, nks in plan]
    pool = rand_keys(rng, 10_001)
    for calls in host:  # the same keys again in every call
        for keys, _ in calls:
            keys[::7] = pool[:keys[::7].size]
    v = _ctx()
    dev = [[(torch.from_numpy(k.view(np.int64)).cuda(), torch.from_numpy(c.view(np.int32)).cuda())
            for k, c in calls] for calls in host]
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    for (k, _), calls, dcalls in zip(plan, host, dev):
        _lib.check(v._L.psg_freq_resize(v._h, ch, n, k))
        t, nn, kk = O.cm_resize(n, k)
        for i, ((keys, counts), (dk, dc)) in enumerate(zip(calls, dcalls)):
            _lib.check(v._L.psg_freq_insert_dev(v._h, ch, dk.data_ptr(), dc.data_ptr(), keys.size,
                                                C.c_void_p(s1.cuda_stream)))
            O.cm_insert(t, nn, kk, keys, counts)
            if check_each or i == len(calls) - 1:
                assert np.array_equal(_table(v, ch, nn), t), (k, i)
    torch.cuda.synchronize()
    v.close()


def _query_dev(v, ch, dkeys, nk, freq, dout, dn, scratch):
    from parameter_server_amd import _lib
    _lib.check(v._L.psg_freq_query_dev(v._h, ch, dkeys.data_ptr() if nk else None, nk, freq,
                                       dout.data_ptr(), dn.data_ptr(), scratch.data_ptr(), None))
    return int(dn.item())


SENTINEL = -0x0123456789ABCDEF
GUARD = 4096


def _query_cases_on_one_table(cases, ch=5):
    """The cases share (n, k): one filter, its table assigned once; every case
    through psg_freq_query, and those marked dev through psg_freq_query_dev
    with caller scratch of exactly psg_freq_query_scratch_bytes(nk) stale
    bytes (0xFF, not refilled between thresholds; the bytes after it must
    stay 0xFF) and `out` holding a sentinel that must survive past nout."""
    import torch
    from parameter_server_amd import _lib
    n, k = cases[0].n, cases[0].k
    assert all((c.n, c.k) == (n, k) for c in cases)
    v = _ctx()
    _lib.check(v._L.psg_freq_resize(v._h, ch, n, k))
    t = q_table(n, k)
    _lib.check(v._L.psg_freq_table_assign(v._h, ch, t.ctypes.data, n))
    assert np.array_equal(_table(v, ch, n), t)
    for c in cases:
        keys, want = q_keys(c.tag), q_expect(c.tag)
        for f in q_freqs(c.tag):
            assert np.array_equal(_query(v, ch, keys, f), want[f]), (c.tag, f)
        if not c.dev:
            continue
        sb = v._L.psg_freq_query_scratch_bytes(c.nk)
        buf = torch.full((sb + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        dk = torch.from_numpy(keys.view(np.int64)).cuda()
        dn = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        for f in q_freqs(c.tag):
            dout = torch.full((c.nk + 64,), SENTINEL, dtype=torch.int64, device="cuda")
            m = _query_dev(v, ch, dk, c.nk, f, dout, dn, buf)
            assert m == want[f].size, (c.tag, f)
            got = dout.cpu().numpy()
            assert np.array_equal(got[:m].view(np.uint64), want[f]), (c.tag, f)
            assert (got[m:] == SENTINEL).all(), (c.tag, f)
        assert bool((buf[sb:] == 0xFF).all()), c.tag
    v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 4, 5, 8])
def test_gpu_query_tile_and_block_edges(k):
    """Query case 1: key counts around the 2048-key compaction tile and the
    4096 / 8192-key blocks, three regions.  (At k = 1 the counts up to 4096
    take the direct form: 4096 * 64 is 4 bytes short of the table.)"""
    _query_cases_on_one_table([c for c in Q_CASES if c.tag.startswith("edge-k%d-" % k)])


@pytest.mark.gpu
def test_gpu_query_form_switch():
    """Query case 2: 1, 100, 2049 and 11,718 keys direct, 11,719 and 12,289 binned."""
    _query_cases_on_one_table([c for c in Q_CASES if c.tag.startswith("switch-")])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 30])
def test_gpu_query_k_above_8_many_regions(k):
    """Query case 3."""
    _query_cases_on_one_table([Q_BY_TAG["bigk-k%d" % k]])


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [c.tag for c in Q_CASES if c.tag.startswith("run-")])
def test_gpu_query_long_runs_and_region_count_edges(tag):
    """Query case 4: a block whose 32768 records fall into one region's run
    (all keys equal; or a table of one region and a few bytes), and tables
    of a region less one byte, exact, plus one."""
    _query_cases_on_one_table([Q_BY_TAG[tag]])


@pytest.mark.gpu
def test_gpu_query_dev_with_no_keys():
    """Query case 5: psg_freq_query_dev with n = 0 after a non-empty query on
    the same scratch: OK, nout = 0, out untouched."""
    import torch
    from parameter_server_amd import _lib
    c = Q_BY_TAG["edge-k4-nk2049"]
    v = _ctx()
    _lib.check(v._L.psg_freq_resize(v._h, 2, c.n, c.k))
    _lib.check(v._L.psg_freq_table_assign(v._h, 2, q_table(c.n, c.k).ctypes.data, c.n))
    sb = v._L.psg_freq_query_scratch_bytes(c.nk)
    assert v._L.psg_freq_query_scratch_bytes(0) <= sb
    buf = torch.full((sb + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    dk = torch.from_numpy(q_keys(c.tag).view(np.int64)).cuda()
    dn = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    dout = torch.full((c.nk + 64,), SENTINEL, dtype=torch.int64, device="cuda")
    f = q_freqs(c.tag)[2]
    want = q_expect(c.tag)[f]
    assert 0 < want.size < c.nk
    assert _query_dev(v, 2, dk, c.nk, f, dout, dn, buf) == want.size
    assert np.array_equal(dout[:want.size].cpu().numpy().view(np.uint64), want)
    dout.fill_(SENTINEL)
    assert _query_dev(v, 2, dk, 0, f, dout, dn, buf) == 0
    assert bool((dout == SENTINEL).all())
    assert bool((buf[sb:] == 0xFF).all())
    v.close()


@pytest.mark.gpu
def test_gpu_insert_then_query():
    """Query case 6: the table the binned insert built (repeated keys, byte
    wrap), then the binned query of the same keys."""
    from parameter_server_amd import _lib
    keys, counts, t, want = insert_then_query_case()
    assert q_is_binned(QN, 5, keys.size)
    v = _ctx()
    _lib.check(v._L.psg_freq_resize(v._h, 1, QN, 5))
    _lib.check(v._L.psg_freq_insert(v._h, 1, keys.ctypes.data, counts.ctypes.data, keys.size))
    assert np.array_equal(_table(v, 1, QN), t)
    for f, w in want.items():
        assert np.array_equal(_query(v, 1, keys, f), w), f
    v.close()


# ------------------------------------------------------------------ CPU --
def _kept_fractions_ok(nk, distinct, kept):
    """kept: {threshold: count}.  -1 keeps everything.  With more than one
    distinct key at least two thresholds keep more than 5 % and fewer than
    95 %.  One distinct key is kept whole or not at all: then some threshold
    other than -1 must keep it and some must drop it."""
    assert kept[-1] == nk
    if distinct > 1:
        return sum(0.05 * nk < m < 0.95 * nk for m in kept.values()) >= 2
    rest = [m for f, m in kept.items() if f != -1]
    return nk in rest and 0 in rest


@pytest.mark.parametrize("tag", [c.tag for c in Q_CASES])
def test_query_case_thresholds_keep_a_real_fraction(tag):
    c = Q_BY_TAG[tag]
    kept = {f: w.size for f, w in q_expect(tag).items()}
    assert {-1, 0, 254} <= set(kept)
    assert _kept_fractions_ok(c.nk, np.unique(q_keys(tag)).size, kept), kept
    assert np.array_equal(q_expect(tag)[-1], q_keys(tag))


def test_insert_then_query_case_thresholds_keep_a_real_fraction():
    keys, _, _, want = insert_then_query_case()
    kept = {f: w.size for f, w in want.items()}
    assert _kept_fractions_ok(keys.size, np.unique(keys).size, kept), kept
    assert np.unique(keys).size < keys.size


def test_query_cases_straddle_the_form_switch():
    forms = {(c.k, q_is_binned(c.n, c.k, c.nk)) for c in Q_CASES}
    assert any((k, True) in forms and (k, False) in forms for k in range(1, Q_MAX_K + 1))
    want = {1: False, 100: False, 2049: False, 11_718: False, 11_719: True, 12_289: True}
    assert {c.nk: q_is_binned(c.n, c.k, c.nk) for c in Q_CASES if c.tag.startswith("switch-")} == want
    assert not any(q_is_binned(c.n, c.k, c.nk) for c in Q_CASES if c.tag.startswith("bigk-"))
    # tiles and blocks: a key count on each side of every multiple that matters
    for k in (1, 4, 5, 8):
        nks = {c.nk for c in Q_CASES if c.tag.startswith("edge-k%d-" % k)}
        for edge in (Q_TILE, 2 * Q_TILE, q_block_keys(k), 8192):
            assert {edge - 1, edge, edge + 1} <= nks
        assert any(nk > 2 * q_block_keys(k) and nk % Q_TILE for nk in nks)
    regions = {q_regions(c.n) for c in Q_CASES}
    assert {1, 2, 3} <= regions and max(regions) > 16


def test_insert_cases_reach_the_edges_they_name():
    shapes = insert_shapes()
    nbs = {(nk + ins_block_keys(k) - 1) // ins_block_keys(k) for _, k, nk in shapes}
    assert {APPLY_WAVE_BLOCKS, APPLY_WAVE_BLOCKS + 1, APPLY_TRIP, APPLY_TRIP + 1} <= nbs
    # the transpose: blocks and region-start columns on both sides of a tile, together
    tr = {((nk + 8192 - 1) // 8192, ins_regions(n) + 1) for n, k, nk in shapes if k == 4}
    for nb in (TRANSPOSE_TILE, TRANSPOSE_TILE + 1):
        for nc in (TRANSPOSE_TILE, TRANSPOSE_TILE + 1):
            assert (nb, nc) in tr
    # k > 8 on more than one region; every block size
    assert any(k > 8 and ins_regions(n) > 1 for n, k, _ in shapes)
    assert {ins_block_keys(k) for _, k, _ in shapes} == {8192, 4096, 2048, 1024}
    assert {1, 2, 3} <= {ins_regions(n) for n, _, _ in shapes}
    assert any(n % 4 for n, _, _ in shapes)
    # a block of exactly 32768 records (records: keys whose count is nonzero mod 2^8, times k)
    full = set()
    for case in [case_k_switch(k, nk) for k, nk in K_SWITCHES] + [case_repeats()]:
        n, k, calls = case
        kb = ins_block_keys(k)
        for keys, counts in calls:
            live = (counts & 0xFF) != 0
            recs = [int(live[b:b + kb].sum()) * k for b in range(0, keys.size, kb)]
            assert max(recs) <= INS_BLOCK_RECS
            if INS_BLOCK_RECS in recs:
                full.add(k)
    assert {4, 8, 16} <= full
    # repeats inside one call, in one block and across blocks
    keys = case_repeats()[2][0][0]
    assert np.unique(keys[:8192]).size == 1 and keys[0] in keys[8192:16384] and keys[0] in keys[16384:]
    keys, counts = case_repeats()[2][2]
    assert np.unique(keys[:8192]).size == 1 and int(counts[:8192].sum()) % 256 != 0
