"""GPU: the feature groups of a loaded minibatch (psg_mb_set_slots,
psg_mb_groups, psg_mb_group_extract) against numpy, at the sort's tile edges
(T = psg_mb_sort_tile()), the 256-row block edges and the key range's ends.
Everything is integer or a copy, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from parameter_server_amd import _lib, slots
from parameter_server_amd.kv_vector import KVVector
from parameter_server_amd.worker import Minibatch, sort_tile

pytestmark = pytest.mark.gpu

KMAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    v = KVVector(0, _lib.PSG_F64)
    yield v
    v.close()


@pytest.fixture(scope="module")
def mbs(ctx):
    src, dst = Minibatch(ctx._h), Minibatch(ctx._h)
    yield src, dst
    src.close()
    dst.close()


# ---- numpy's side -------------------------------------------------------------------
def build(rows_spec, valued, seed=1, keys=None):
    """rows_spec: per row a list of (slot id, entries) runs.  Random keys
    (or `keys`, consumed in order) and values."""
    rng = np.random.default_rng(seed)
    offset, slot = [0], []
    for runs in rows_spec:
        for s, k in runs:
            slot += [s] * k
        offset.append(len(slot))
    n = len(slot)
    index = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n, dtype=np.uint64)
    if keys is not None:
        index[:len(keys)] = np.array(keys, dtype=np.uint64)
    value = rng.standard_normal(n) if valued else None
    y = rng.choice([-1.0, 1.0], len(rows_spec))
    return (np.array(offset, np.uint64), index, value, y, np.array(slot, np.uint16))


def np_bad_row(offset, slot):
    for r in range(offset.size - 1):
        s = slot[int(offset[r]):int(offset[r + 1])].astype(np.int64)
        if s.size == 0:
            continue
        heads = s[np.r_[True, s[1:] != s[:-1]]]
        if np.unique(heads).size != heads.size or s.min() < 1 or s.max() > 4095:
            return r
    return -1


def np_info(offset, index, slot, valued):
    rows = offset.size - 1
    row_of = np.repeat(np.arange(rows), np.diff(offset).astype(np.int64))
    out = []
    if rows:
        out.append({"id": 0, "format": 1, "min_key": 0, "max_key": 1, "nnz_ele": rows,
                    "nnz_ex": rows})
    for s in np.unique(slot):
        m = slot == s
        k = index[m]
        out.append({"id": int(s), "format": 2 if valued else 3, "min_key": int(k.min()),
                    "max_key": int((k + np.uint64(1)).max()),  # wraps, as written
                    "nnz_ele": int(m.sum()),
                    "nnz_ex": rows if valued and s == 1 else int(np.unique(row_of[m]).size)})
    return out


def np_extract(offset, index, value, slot, s):
    m = slot == s
    before = np.r_[0, np.cumsum(m)].astype(np.uint64)
    return before[offset.astype(np.int64)], index[m], None if value is None else value[m]


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def load(mb, data):
    offset, index, value, y, slot = data
    mb.load(offset, index, value, y)
    slots.mb_set_slots(mb, slot)


def check(mbs, data, extra_slots=(3000,), only=None):
    """groups and the extraction of every slot present (or of `only`) and of
    absent ones against numpy."""
    src, dst = mbs
    offset, index, value, y, slot = data
    assert np_bad_row(offset, slot) == -1
    load(src, data)
    assert same(src.read("slot"), slot)
    info, bad = slots.mb_groups(src)
    assert bad == -1
    want = np_info(offset, index, slot, value is not None)
    assert info == want
    again, _ = slots.mb_groups(src)  # the same bytes on every run
    assert again == info
    present = [i["id"] for i in want if i["id"]]
    for s in (present if only is None else list(only)) + list(extra_slots):
        slots.mb_group_extract(src, s, dst)
        o, i, v = np_extract(offset, index, value, slot, s)
        assert same(dst.read("offset"), o), s
        assert same(dst.read("index"), i), s
        if value is not None:
            assert same(dst.read("value"), v), s
        else:
            assert dst.read("value").size == 0
        assert same(dst.read("y"), y), s
    return info


def two_slot_rows(a, b, nnz):
    """Rows of [a x 3, b x 4] with empty rows first, in the middle and last,
    rows of one slot only, and a tail so that the entries are exactly nnz."""
    spec = [[], []]
    left = nnz
    r = 0
    while left >= 7:
        spec.append([(a, 3), (b, 4)] if r % 5 else ([(b, 7)] if r % 2 else [(a, 7)]))
        left -= 7
        r += 1
        if r == 11:
            spec += [[], []]
    if left:
        spec.append([(b, left)])
    return spec + [[]]


# ---- cases -------------------------------------------------------------------------
def test_no_rows_and_no_entries(mbs):
    src, dst = mbs
    empty = build([], False)
    assert check(mbs, empty, extra_slots=(1,)) == []
    info = check(mbs, build([[], [], [], [], []], True), extra_slots=(1, 4095))
    assert [i["id"] for i in info] == [0] and dst.rows == 5


@pytest.mark.parametrize("valued", (False, True))
def test_one_group(mbs, valued):
    T = sort_tile()
    info = check(mbs, build([[(7, 5)]] * (T // 5) + [[(7, T + 1 - 5 * (T // 5))]], valued))
    assert [i["id"] for i in info] == [0, 7] and info[1]["nnz_ele"] == T + 1


@pytest.mark.parametrize("ids", ((1, 2), (1, 257), (2, 4095)))
@pytest.mark.parametrize("dn", ("T-1", "T", "T+1", "2T+1"))
def test_two_groups_around_the_tile(mbs, ids, dn):
    T = sort_tile()
    nnz = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[dn]
    data = build(two_slot_rows(*ids, nnz), valued=(dn == "T"))
    offset, slot = data[0], data[4]
    assert slot.size == nnz
    if nnz > T:  # a run of one slot in one row crosses the tile boundary
        r = int(np.searchsorted(offset, T, side="right")) - 1
        assert offset[r] < T and slot[T - 1] == slot[T]
    info = check(mbs, data)
    assert [i["id"] for i in info] == [0, *ids]


def test_segment_ends_at_the_tile_boundary(mbs):
    T = sort_tile()
    data = build([[(5, 1), (300, 1)]] * T + [[(300, 1)]], False)  # T entries of slot 5
    info = check(mbs, data)
    assert info[1]["nnz_ele"] == T and info[2]["nnz_ele"] == T + 1


@pytest.mark.parametrize("rows", (255, 256, 257))
def test_rows_around_a_block(mbs, rows):
    spec = [[(2, 1), (9, 2)] if r % 3 else [(9, 1)] for r in range(rows)]
    spec[rows // 2] = [(2, 1), (9, 1), (1000, 4)]  # a group present in a single row
    info = check(mbs, build(spec, rows == 256))
    assert info[3]["id"] == 1000 and info[3]["nnz_ex"] == 1 and info[0]["nnz_ex"] == rows


@pytest.mark.parametrize("valued", (False, True))
def test_key_range_ends(mbs, valued):
    data = build([[(1, 2), (4, 2)], [(4, 1)], [(6, 1)]], valued, keys=[0, KMAX, 5, 0, KMAX, KMAX])
    info = check(mbs, data)
    assert (info[1]["min_key"], info[1]["max_key"]) == (0, 1)   # {0, 2^64 - 1}: max of {1, 0}
    assert (info[2]["min_key"], info[2]["max_key"]) == (0, 6)   # {5, 0, 2^64 - 1}
    assert (info[3]["min_key"], info[3]["max_key"]) == (KMAX, 0)
    if valued:
        assert info[1]["nnz_ex"] == 3 and info[2]["nnz_ex"] == 2  # slot 1: every row


def test_same_id_across_a_row_boundary_is_legal(mbs):
    check(mbs, build([[(3, 2), (8, 2)], [(8, 3), (3, 1)], [(3, 2)], [], [(3, 1)]], False))


def bad_row_of(mbs, data):
    src, dst = mbs
    load(src, data)
    info, bad = slots.mb_groups(src)
    assert bad == np_bad_row(data[0], data[4]) and bad >= 0 and info == []
    with pytest.raises(_lib.PSGError) as e:  # no extraction after a bad row
        slots.mb_group_extract(src, 1, dst)
    assert e.value.status == _lib.PSG_ERR_ARG
    return bad


def test_split_ids(mbs):
    T = sort_tile()
    ok = [(1, 2), (2, 2)]
    assert bad_row_of(mbs, build([[(1, 1), (2, 1), (1, 1)], ok, ok], False)) == 0
    assert bad_row_of(mbs, build([ok, ok, [(2, 1), (1, 2), (2, 3)]], False)) == 2
    # the two runs in different tiles of the sort
    assert bad_row_of(mbs, build([ok, [(1, 10), (2, T), (1, 10)], ok], True)) == 1
    # two bad rows: the smaller one
    spec = [ok] * 700 + [[(1, 1), (2, 1), (1, 1)]] + [ok] * 300 + [[(2, 1), (1, 1), (2, 1)]]
    assert bad_row_of(mbs, build(spec, False)) == 700
    assert bad_row_of(mbs, build(spec[::-1], False)) == 0


@pytest.mark.parametrize("bad_id", (0, 4096, 65535))
def test_ids_out_of_range(mbs, bad_id):
    ok = [(1, 2), (2, 2)]
    assert bad_row_of(mbs, build([ok, ok, [(1, 1), (bad_id, 2)], ok], False)) == 2


def test_many_distinct_ids(mbs):
    """4095 slots, one entry each, and more ids than slots exist."""
    info = check(mbs, build([[(s, 1) for s in range(4095, 0, -1)]], False), extra_slots=(),
                 only=(1, 255, 256, 4095))
    assert len(info) == 4096
    load(mbs[0], build([[(s, 1) for s in range(1, 5001)]], False))
    assert slots.mb_groups(mbs[0]) == ([], 0)


def test_errors(ctx, mbs):
    src, dst = mbs
    L = _lib.lib()
    data = build([[(1, 2), (2, 2)], [(2, 1)]], False)

    def status(f, *a):
        with pytest.raises(_lib.PSGError) as e:
            f(*a)
        return e.value.status

    src.load(*data[:4])
    assert status(slots.mb_groups, src) == _lib.PSG_ERR_ARG          # no slot ids yet
    assert status(src.read, "slot") == _lib.PSG_ERR_ARG
    assert status(slots.mb_set_slots, src, data[4][:3]) == _lib.PSG_ERR_SIZE
    slots.mb_set_slots(src, data[4])
    assert status(slots.mb_group_extract, src, 1, dst) == _lib.PSG_ERR_ARG  # before psg_mb_groups
    n, bad = C.c_size_t(), C.c_int64()
    assert L.psg_mb_groups(src._h, None, 2, C.byref(n), C.byref(bad)) == _lib.PSG_ERR_SIZE
    assert n.value == 3
    slots.mb_groups(src)
    assert status(slots.mb_group_extract, src, 1, src) == _lib.PSG_ERR_ARG
    assert status(slots.mb_group_extract, src, 0, dst) == _lib.PSG_ERR_ARG
    assert status(slots.mb_group_extract, src, 4096, dst) == _lib.PSG_ERR_ARG
    other = KVVector(0, _lib.PSG_F64)
    far = Minibatch(other._h)
    try:
        assert status(slots.mb_group_extract, src, 1, far) == _lib.PSG_ERR_ARG  # two contexts
    finally:
        far.close()
        other.close()
    slots.mb_group_extract(src, 2, dst)
    assert dst.read("offset").tolist() == [0, 2, 3]
    # the loaded source is still a minibatch: its own uniq works, and reuses the sort's blocks
    assert src.uniq() == np.unique(data[1]).size
    assert status(slots.mb_group_extract, src, 1, dst) == _lib.PSG_ERR_ARG
    assert status(slots.mb_groups, src) == _lib.PSG_ERR_ARG
    assert status(slots.mb_set_slots, src, data[4]) == _lib.PSG_ERR_ARG
    # a new load drops the slot ids
    src.load(*data[:4])
    assert status(slots.mb_groups, src) == _lib.PSG_ERR_ARG
    # the extracted minibatch is a loaded one
    assert dst.uniq() == np.unique(data[1][data[4] == 2]).size
