"""GPU: checkpoint and restore of the resident FTRL model (psg_ftrl_import,
psg_ftrl_export_state, psg_ftrl_frozen, psg_freq_table_assign and their
Python mirrors) against the CPU restatement of the model (tests/ftrl_ref.py).
Every comparison is by bits."""
import ctypes as C
import os

import numpy as np
import pytest

import auc_ref as A
import ftrl_ref as R
import worker_ref as W
from parameter_server_amd import _lib
from parameter_server_amd.ftrl import FTRLModel, read_model_text
from parameter_server_amd.worker import (FTRLWorker, evaluate_model, parse_text_host, sort_tile)

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
NAMES = ("keys", "pos", "neg", "w", "z")
DTYPES = (np.uint64, np.uint64, np.uint64, np.float64, np.float64)


def ptr(a):
    return None if a is None else a.ctypes.data


def new_model(hint=0, **param):
    p = dict(R.PARITY_PARAM, **param)
    m = FTRLModel(0, capacity_hint=hint)
    m.setLearningRate(p["alpha"], p["beta"])
    m.setPenalty(p["lambda1"], p["lambda2"])
    m._model()
    return m


def push(m, keys, pos, neg, grad):
    """psg_ftrl_push with the status returned, not raised."""
    k = np.ascontiguousarray(keys, np.uint64)
    a, b = np.ascontiguousarray(pos, np.uint32), np.ascontiguousarray(neg, np.uint32)
    g = np.ascontiguousarray(grad, np.float64)
    return m._L.psg_ftrl_push(m._h, ptr(k), k.size, ptr(a), ptr(b), ptr(g))


def imp(m, keys, pos, neg, w, z):
    """psg_ftrl_import with the status returned, not raised."""
    a = [None if x is None else np.ascontiguousarray(x, dt)
         for x, dt in zip((keys, pos, neg, w, z), DTYPES)]
    return m._L.psg_ftrl_import(m._h, ptr(a[0]), a[0].size, ptr(a[1]), ptr(a[2]), ptr(a[3]),
                                ptr(a[4]))


def status(m):
    e, z = C.c_size_t(), C.c_size_t()
    n1, n2 = C.c_double(), C.c_double()
    rc = m._L.psg_ftrl_status(m._h, C.byref(e), C.byref(z), C.byref(n1), C.byref(n2))
    return rc, e.value, z.value, n1.value, n2.value


def same(got, want, what=""):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES + ("found",), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, name)


def image_of(ref):
    """The whole state of a VectorFTRL: its entries by key, zero weights too."""
    return ref.keys, ref.pos, ref.neg, ref.w, ref.z


def ref_of(image):
    """A VectorFTRL that holds `image`."""
    ref = R.VectorFTRL(**R.PARITY_PARAM)
    ref.keys, ref.pos, ref.neg, ref.w, ref.z = (np.array(a, dt) for a, dt in zip(image, DTYPES))
    ref.nnz = int(np.count_nonzero(ref.w != 0))
    return ref


def upsert(ref, keys, pos, neg, w, z):
    """psg_ftrl_import restated: whole entries replace or join those of ref."""
    old = dict(zip(ref.keys.tolist(), zip(ref.pos.tolist(), ref.neg.tolist(),
                                          R.bits(ref.w).tolist(), R.bits(ref.z).tolist())))
    n = len(keys)
    pos = np.zeros(n, np.uint64) if pos is None else pos
    neg = np.zeros(n, np.uint64) if neg is None else neg
    z = np.zeros(n, np.float64) if z is None else z
    old.update(zip(np.asarray(keys, np.uint64).tolist(),
                   zip(np.asarray(pos, np.uint64).tolist(), np.asarray(neg, np.uint64).tolist(),
                       R.bits(w).tolist(), R.bits(z).tolist())))
    ks = sorted(old)
    ref.keys = np.array(ks, np.uint64)
    ref.pos = np.array([old[k][0] for k in ks], np.uint64)
    ref.neg = np.array([old[k][1] for k in ks], np.uint64)
    ref.w = np.array([old[k][2] for k in ks], np.uint64).view(np.float64)
    ref.z = np.array([old[k][3] for k in ks], np.uint64).view(np.float64)
    ref.nnz = int(np.count_nonzero(ref.w != 0))


def random_image(rng, keys):
    """Whole entries for `keys` (sorted unique): counts past 2^32 among them,
    a third of the weights +0.0 or -0.0."""
    n = keys.size
    pos = rng.integers(0, 1 << 34, size=n, dtype=np.uint64)
    neg = rng.integers(0, 50, size=n, dtype=np.uint64)
    w = rng.standard_normal(n)
    w[rng.random(n) < 1 / 6] = 0.0
    w[rng.random(n) < 1 / 6] = -0.0
    return keys, pos, neg, w, 3.0 * rng.standard_normal(n)


@pytest.fixture(scope="module")
def parity():
    """The parity case and its restatement after three and six messages (read only)."""
    uni, msgs = R.parity_case(seed=1)
    ref = R.VectorFTRL(**R.PARITY_PARAM)
    for msg in msgs[:3]:
        ref.push(*msg)
    half = tuple(a.copy() for a in image_of(ref))
    for msg in msgs[3:]:
        ref.push(*msg)
    return uni, msgs, ref, half


# ------------------------------------------------------------------- resume --
def test_resume_from_a_saved_state(parity):
    uni, msgs, ref, half = parity
    a = new_model(hint=64)
    for msg in msgs[:3]:
        assert push(a, *msg) == _lib.PSG_OK
    st = a.state()
    same(st, half, "the state after three messages")
    b = new_model(hint=64)
    b.restore(*st)
    for msg in msgs[3:]:
        assert push(a, *msg) == _lib.PSG_OK
        assert push(b, *msg) == _lib.PSG_OK
    keys = np.concatenate([uni, R.absent_keys(uni, 500)])
    la, lb, lr = a.lookup(keys), b.lookup(keys), ref.lookup(keys)
    same((keys,) + la, (keys,) + lr, "uninterrupted")
    same((keys,) + lb, (keys,) + lr, "resumed")
    (rca, ea, za, n1a, n2a), (rcb, eb, zb, n1b, n2b) = status(a), status(b)
    assert rca == rcb == _lib.PSG_OK
    assert ea == eb == ref.entries and za == zb == ref.nnz and za > 0
    # psg.h: each model's norm is within entries * 2^-53 * (the sum) of the sum
    assert n1a > 0 and n2a > 0
    assert abs(n1a - n1b) <= 2 * ea * 2.0 ** -53 * n1a
    assert abs(n2a - n2b) <= 2 * ea * 2.0 ** -53 * n2a
    same(a.state(), b.state(), "the two images")
    a.close()
    b.close()


# -------------------------------------------------------------------- image --
def test_image_is_sorted_whole_and_independent_of_the_table(parity):
    uni, msgs, ref, _ = parity
    small = new_model(hint=64)           # rehashed as the messages come
    for msg in msgs:
        assert push(small, *msg) == _lib.PSG_OK
    st = small.state()
    assert st[0].size == ref.entries and np.all(st[0][1:] > st[0][:-1])
    same(st, image_of(ref), "against the restatement")
    assert int(np.count_nonzero(st[3] == 0)) >= 1       # entries with w == +-0 are in it
    assert int(np.count_nonzero(R.bits(st[3]) == R.bits([-0.0])[0])) >= 1
    big = new_model(hint=1 << 20)        # another table size, other slots, one import
    big.restore(*st)
    again = big.state()
    for name, x, y in zip(NAMES, st, again):
        assert x.tobytes() == y.tobytes(), name
    same(small.state(), st, "the same bytes on every run")
    assert status(big)[1:3] == status(small)[1:3] == (ref.entries, ref.nnz)
    small.close()
    big.close()


def test_edge_keys_and_values_survive_bit_for_bit():
    nan = np.array([0x7ff8000000000123, 0xfff4000000000001], np.uint64).view(np.float64)
    keys = np.array([0, 1, 1 << 63, U64], np.uint64)
    pos = np.array([(1 << 32) + 5, 0, U64, 7], np.uint64)
    neg = np.array([3, 1 << 40, 0, (1 << 32) - 1], np.uint64)
    w = np.array([-0.0, nan[0], 1.5, -0.0])
    z = np.array([nan[1], -0.0, np.inf, 3.0])
    m = new_model(hint=16)
    m.restore(keys, pos, neg, w, z)
    same(m.state(), (keys, pos, neg, w, z))
    same((keys,) + m.lookup(keys), (keys, pos, neg, w, z, np.ones(4, np.uint8)))
    # ftrl_model.h:106-110's comparisons: -0.0 is zero, a NaN weight is not
    assert status(m)[:3] == (_lib.PSG_OK, 4, 2)
    assert not m.frozen
    m.close()


# ------------------------------------------------------------------- upsert --
def test_upsert_replaces_inserts_and_counts():
    rng = np.random.default_rng(11)
    K = np.unique(np.concatenate([rng.integers(0, 1 << 64, size=598, dtype=np.uint64),
                                  np.array([0, U64], np.uint64)]))
    assert K.size == 600
    first = list(random_image(rng, K[:400]))
    second = list(random_image(rng, K[200:]))
    i = np.arange(400)
    first[3] = np.where(i % 2 == 0, np.where(i % 4 == 0, 0.0, -0.0), first[3] + 4.0)
    second[3] = np.where((i // 2) % 2 == 0, np.where(i % 3 == 0, 0.0, -0.0), second[3] + 4.0)
    kinds = dict.fromkeys(R.TRANSITIONS, 0)
    for old, new in zip(first[3][200:].tolist(), second[3][:200].tolist()):
        kinds[R._kind(new, old)] += 1
    assert all(kinds[k] >= 1 for k in R.TRANSITIONS), kinds
    m, ref = new_model(hint=64), ref_of([a[:0] for a in first])
    m.restore(*first)
    upsert(ref, *first)
    assert status(m)[:3] == (_lib.PSG_OK, 400, ref.nnz)
    m.restore(*second)                   # 200 keys present, 200 not yet
    upsert(ref, *second)
    assert ref.entries == 600 and 0 < ref.nnz < 600
    assert status(m)[:3] == (_lib.PSG_OK, 600, ref.nnz)
    same(m.state(), image_of(ref), "after the overlapping import")
    assert not m.frozen
    # weights-only over whole entries: (0, 0, w, +0.0)
    k3, w3 = K[100:300], second[3][:200][::-1].copy()
    m.restore(k3, w=w3)
    upsert(ref, k3, None, None, w3, None)
    st = m.state()
    same(st, image_of(ref), "after the weights-only import")
    at = np.isin(st[0], k3)
    assert not st[1][at].any() and not st[2][at].any() and not R.bits(st[4][at]).any()
    assert st[1][~at].any() and R.bits(st[4][~at]).any()
    assert status(m)[:3] == (_lib.PSG_OK, 600, ref.nnz)
    assert m.frozen
    m.close()


# ------------------------------------------------------------------- growth --
def test_an_import_larger_than_the_table_grows_it(parity):
    uni, msgs, _, _ = parity
    rng = np.random.default_rng(12)
    img = random_image(rng, uni)
    assert uni.size == 3000
    m, ref = new_model(hint=64), ref_of(img)
    m.restore(*img)
    same(m.state(), img)
    assert status(m)[:3] == (_lib.PSG_OK, 3000, ref.nnz)
    for msg in msgs[:2]:                 # the same model then accepts pushes
        assert push(m, *msg) == _lib.PSG_OK
        ref.push(*msg)
    keys = np.concatenate([uni, R.absent_keys(uni, 100)])
    same((keys,) + m.lookup(keys), (keys,) + ref.lookup(keys))
    assert status(m)[:3] == (_lib.PSG_OK, ref.entries, ref.nnz)
    m.close()


# -------------------------------------------------------------------- range --
def test_closed_key_ranges():
    rng = np.random.default_rng(13)
    K = np.unique(np.concatenate([rng.integers(0, 1 << 64, size=300, dtype=np.uint64),
                                  np.array([0, 5, 9, U64 - 4, U64], np.uint64)]))
    img = random_image(rng, K)
    m = new_model(hint=64)
    m.restore(*img)

    def want(lo, hi):
        keep = np.array([lo <= k <= hi for k in K.tolist()], bool)
        return tuple(a[keep] for a in img)

    a, b = int(K[40]), int(K[200])
    cases = [(a, b), (a + 1, b - 1), (a, a), (0, 0), (U64, U64), (0, U64), (1, U64 - 1),
             (6, 8), (a + 1, int(K[41]) - 1), (0, a), (b, U64)]
    for lo, hi in cases:
        got = m.state(range=(lo, hi))
        same(got, want(lo, hi), (lo, hi))
    assert m.state(range=(a, b))[0].size == 161 and m.state(range=(a + 1, b - 1))[0].size == 159
    assert m.state(range=(6, 8))[0].size == 0           # an empty result
    assert m.state(range=(0, 0))[0].tolist() == [0]
    assert m.state(range=(U64, U64))[0].tolist() == [U64]
    with pytest.raises(_lib.PSGError) as e:
        m.state(range=(b, a))
    assert e.value.status == _lib.PSG_ERR_ARG
    # two complementary ranges concatenate to the whole image
    for cut in (a, a + 1, 0, U64 - 1):
        lo, hi = m.state(range=(0, cut)), m.state(range=(cut + 1, U64))
        same(tuple(np.concatenate(p) for p in zip(lo, hi)), img, cut)
    m.close()


# --------------------------------------------------------------- sort edges --
def sort_edge_cases():
    tile = sort_tile()
    rng = np.random.default_rng(14)
    cases = {}
    for n in (0, 1, tile - 1, tile, tile + 1, 2 * tile + 1):
        k = np.unique(rng.integers(0, 1 << 64, size=n + 64, dtype=np.uint64))
        cases["n=%d" % n] = rng.permutation(k)[:n]
    cases["one byte"] = W.digits_only(rng, 200, (2,))
    cases["top byte"] = W.digits_only(rng, 200, (7,))
    cases["two bytes past a tile"] = W.digits_only(rng, tile + 300, (0, 5))
    return cases


def test_sort_edges():
    tile = sort_tile()
    rng = np.random.default_rng(15)
    for name, k in sort_edge_cases().items():
        keys = np.unique(k)
        if name.startswith("n="):
            assert keys.size == int(name[2:])
        elif "past a tile" in name:
            assert keys.size > tile
        else:
            assert 100 < keys.size <= 200
            x = np.bitwise_xor.reduce(np.stack([keys, np.roll(keys, 1)]))
            differ = int(np.bitwise_or.reduce(x))
            assert differ and differ & ~(0xFF << (16 if name == "one byte" else 56)) == 0
        img = random_image(rng, keys)
        m = new_model(hint=64)
        m.restore(*img)
        st = m.state()
        same(st, img, name)
        assert status(m)[:2] == (_lib.PSG_OK, keys.size)
        m.close()


# ---------------------------------------------------------------- rejection --
def test_an_unsorted_import_applies_nothing_and_is_reported_once():
    rng = np.random.default_rng(16)
    K = np.unique(rng.integers(1, 1 << 64, size=500, dtype=np.uint64))
    img = random_image(rng, K[:300])
    m = new_model(hint=64)
    m.restore(*img)
    before = m.lookup(K)
    assert status(m)[:2] == (_lib.PSG_OK, 300)
    bad = list(random_image(rng, K[250:450]))
    bad[0] = bad[0].copy()
    bad[0][77] = bad[0][76]              # one equal pair of neighbours
    assert imp(m, *bad) == _lib.PSG_OK   # asynchronous: the device check rejects it
    same((K,) + m.lookup(K), (K,) + before, "nothing applied")
    rc = status(m)
    assert rc[0] == _lib.PSG_ERR_UNSORTED and b"not strictly increasing" in m._L.psg_last_error()
    assert status(m)[:2] == (_lib.PSG_OK, 300)          # reported once
    good = random_image(rng, K[250:450])
    assert imp(m, *good) == _lib.PSG_OK                 # the following import applies
    ref = ref_of(img)
    upsert(ref, *good)
    same(m.state(), image_of(ref))
    assert status(m)[:3] == (_lib.PSG_OK, 450, ref.nnz)
    # a weights-only import is checked alike, and the state export reports too
    assert imp(m, K[:10][::-1].copy(), None, None, np.ones(10), None) == _lib.PSG_OK
    with pytest.raises(_lib.PSGError) as e:
        m.state()
    assert e.value.status == _lib.PSG_ERR_UNSORTED
    same(m.state(), image_of(ref))
    m.close()


# ------------------------------------------------------------- cap protocol --
def test_cap_protocol_and_null_outputs():
    rng = np.random.default_rng(17)
    img = random_image(rng, np.unique(rng.integers(0, 1 << 64, size=100, dtype=np.uint64)))
    m = new_model(hint=64)
    m.restore(*img)
    L, n = m._L, C.c_size_t(12345)
    assert L.psg_ftrl_export_state(m._h, None, None, None, None, None, None, 0,
                                   C.byref(n)) == _lib.PSG_ERR_SIZE
    assert n.value == 100
    out = [np.full(100, 0xAB, dt) for dt in DTYPES]
    sentinel = [a.copy() for a in out]
    n = C.c_size_t(0)
    assert L.psg_ftrl_export_state(m._h, None, *[ptr(a) for a in out], 99,
                                   C.byref(n)) == _lib.PSG_ERR_SIZE
    assert n.value == 100
    for a, s in zip(out, sentinel):
        assert a.tobytes() == s.tobytes()               # nothing copied
    # cap == n, every output NULL: the count alone
    n = C.c_size_t(0)
    assert L.psg_ftrl_export_state(m._h, None, None, None, None, None, None, 100,
                                   C.byref(n)) == _lib.PSG_OK and n.value == 100
    # any subset of the outputs
    for pick in ((0,), (4,), (1, 3), (0, 2, 4)):
        out = [np.full(128, 0xAB, dt) if i in pick else None for i, dt in enumerate(DTYPES)]
        n = C.c_size_t(0)
        assert L.psg_ftrl_export_state(m._h, None, *[ptr(a) for a in out], 128,
                                       C.byref(n)) == _lib.PSG_OK and n.value == 100
        for i in pick:
            assert out[i][:100].tobytes() == np.ascontiguousarray(img[i], DTYPES[i]).tobytes()
            assert out[i][100:].tobytes() == np.full(28, 0xAB, DTYPES[i]).tobytes()
    # a range's count
    r = (C.c_uint64 * 2)(int(img[0][10]), int(img[0][19]))
    assert L.psg_ftrl_export_state(m._h, r, None, None, None, None, None, 5,
                                   C.byref(n)) == _lib.PSG_ERR_SIZE and n.value == 10
    m.close()


# ------------------------------------------------------------- device forms --
def test_device_forms_run_in_call_order_across_streams(parity):
    import torch
    uni, msgs, _, _ = parity
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(18)
    extra = np.unique(np.concatenate([msgs[2][0][::3], R.absent_keys(uni, 400)]))
    img = random_image(rng, extra)       # overlaps the third message's keys

    def put(a, dt):
        a = np.ascontiguousarray(a, dt)
        return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).to(dev)

    dmsgs = [(put(k, np.uint64), put(p, np.uint32), put(q, np.uint32), put(g, np.float64))
             for k, p, q, g in msgs[:3]]
    dimg = [put(a, dt) for a, dt in zip(img, DTYPES)]
    cap = 5000
    outs = [[torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(5)] for _ in range(2)]
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    m = new_model(hint=64)
    m.reserve(8000)
    L, h = m._L, m._h

    def push_dev(d, s):
        _lib.check(L.psg_ftrl_push_dev(h, d[0].data_ptr(), d[0].numel(), d[1].data_ptr(),
                                       d[2].data_ptr(), d[3].data_ptr(), s.cuda_stream))

    def export_dev(i, s):
        _lib.check(L.psg_ftrl_export_state_dev(
            h, None, *[t.data_ptr() for t in outs[i]], cap, counts.data_ptr() + 8 * i,
            s.cuda_stream))

    ref = R.VectorFTRL(**R.PARITY_PARAM)
    push_dev(dmsgs[0], s1)
    ref.push(*msgs[0])
    export_dev(0, s2)
    want0 = tuple(a.copy() for a in image_of(ref))
    push_dev(dmsgs[1], s1)
    ref.push(*msgs[1])
    _lib.check(L.psg_ftrl_import_dev(h, dimg[0].data_ptr(), dimg[0].numel(), dimg[1].data_ptr(),
                                     dimg[2].data_ptr(), dimg[3].data_ptr(), dimg[4].data_ptr(),
                                     s2.cuda_stream))
    upsert(ref, *img)
    push_dev(dmsgs[2], s1)
    ref.push(*msgs[2])
    export_dev(1, s2)
    torch.cuda.synchronize()
    n = counts.cpu().numpy().tolist()
    assert n == [want0[0].size, ref.entries]
    for i, want in enumerate((want0, image_of(ref))):
        got = tuple(t[:n[i]].cpu().numpy().view(dt) for t, dt in zip(outs[i], DTYPES))
        same(got, want, "export %d" % i)
    same(m.state(), image_of(ref))
    assert status(m)[:3] == (_lib.PSG_OK, ref.entries, ref.nnz)
    # cap too small: the count is still written
    small = torch.zeros(1, dtype=torch.int64, device=dev)
    rc = L.psg_ftrl_export_state_dev(h, None, *[t.data_ptr() for t in outs[0]], 10,
                                     small.data_ptr(), s2.cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.PSG_ERR_SIZE and int(small.cpu()[0]) == ref.entries
    m.close()


# ------------------------------------------------------------------- frozen --
def test_a_model_read_from_its_dump_is_frozen(parity, tmp_path):
    uni, msgs, ref, _ = parity
    src = new_model(hint=64)
    for msg in msgs:
        assert push(src, *msg) == _lib.PSG_OK
    path = str(tmp_path / "model.txt")
    src.writeToFile(path)
    src.close()
    keys = np.concatenate([uni, R.absent_keys(uni, 200)])
    w = R.pull(ref, keys)
    rounded = np.array([float("%g" % x) if x != 0 else 0.0 for x in w.tolist()])
    assert np.count_nonzero(rounded != w) > 100 and np.count_nonzero(rounded) == ref.nnz
    for real, want in ((np.float64, rounded),
                       (np.float32, rounded.astype(np.float32).astype(np.float64))):
        m = new_model(hint=64)
        assert not m.frozen
        m.readFromFile(path, real=real)
        from parameter_server_amd.kv_vector import Message
        req = Message(key=keys)
        m.getValue(req)
        assert np.array_equal(R.bits(req.value[0]), R.bits(want)), real
        f = C.c_int(-1)
        assert m._L.psg_ftrl_frozen(m._h, C.byref(f)) == _lib.PSG_OK and f.value == 1
        assert status(m)[:3] == (_lib.PSG_OK, ref.nnz, ref.nnz)
        k, v = m.export()                # exports and lookups work
        held = want[:uni.size] != 0      # uni is sorted, as the export is
        assert np.array_equal(k, uni[held]) and np.array_equal(R.bits(v), R.bits(want[:uni.size][held]))
        assert m.lookup(keys)[4].sum() == ref.nnz
        assert push(m, *msgs[0]) == _lib.PSG_ERR_ARG
        assert b"frozen" in m._L.psg_last_error()
        assert m._L.psg_ftrl_push_dev(m._h, None, 0, None, None, None, None) == _lib.PSG_ERR_ARG
        assert b"frozen" in m._L.psg_last_error()
        wk = FTRLWorker(m)
        batch = W.closed_loop_batches(nbatch=1, rows=20)[0]
        with pytest.raises(_lib.PSGError) as e:
            wk.step(*batch)
        assert e.value.status == _lib.PSG_ERR_ARG
        wk.close()
        same((keys,) + m.lookup(keys)[:4], (keys, np.zeros(keys.size, np.uint64),
                                            np.zeros(keys.size, np.uint64), want,
                                            np.zeros(keys.size)), "refused pushes apply nothing")
        # psg_ftrl_init: a fresh, unfrozen model
        p = _lib.FtrlParam(*[R.PARITY_PARAM[k] for k in ("alpha", "beta", "lambda1", "lambda2")])
        _lib.check(m._L.psg_ftrl_init(m._h, C.byref(p), 64))
        assert m._L.psg_ftrl_frozen(m._h, C.byref(f)) == _lib.PSG_OK and f.value == 0
        assert push(m, *msgs[0]) == _lib.PSG_OK
        one = R.VectorFTRL(**R.PARITY_PARAM)
        one.push(*msgs[0])
        same(m.state(), image_of(one), "pushes apply after init")
        m.close()


# ------------------------------------------------------------------- worker --
def test_worker_save_and_load_resume_with_the_same_bits(tmp_path):
    batches = W.closed_loop_batches(seed=29, nbatch=4, rows=100, mean=8, universe=300)

    def worker():
        m = new_model(hint=64, alpha=0.1)
        return FTRLWorker(m, tail_feature_freq=2, countmin_n=64, countmin_k=2)

    whole = worker()
    for b in batches:
        whole.step(*b)
    first = worker()
    for b in batches[:2]:
        first.step(*b)
    path = str(tmp_path / "worker.ckpt")
    first.save(path)
    assert os.path.exists(path)
    mid_state, mid_table = first.model.state(), first.freq_table()
    first.close()
    first.model.close()
    resumed = FTRLWorker.load(path)
    same(resumed.model.state(), mid_state, "loaded")
    assert resumed.freq_table().tobytes() == mid_table.tobytes() and mid_table.any()
    assert (resumed.freq, resumed.countmin_n, resumed.countmin_k) == (2, 64, 2)
    assert (resumed.model._alpha, resumed.model._lambda1) == (0.1, R.PARITY_PARAM["lambda1"])
    for b in batches[2:]:
        resumed.step(*b)
    assert 0 < whole.ndict <= whole.mb.n_uniq
    same(resumed.model.state(), whole.model.state(), "after four minibatches")
    assert whole.model.state()[0].size > 50
    assert resumed.freq_table().tobytes() == whole.freq_table().tobytes()
    assert R.bits(resumed.objv).tolist() == R.bits(whole.objv).tolist() and whole.objv > 0
    assert resumed.num_ex == whole.num_ex == 400
    assert resumed.last_w().tobytes() == whole.last_w().tobytes() and whole.last_w().any()
    assert status(resumed.model)[1:3] == status(whole.model)[1:3]
    # the table's inverse checks its size
    L, ctx = resumed._L, resumed._ctx
    t = np.zeros(128, np.uint8)
    assert L.psg_freq_table_assign(ctx, 0, ptr(t), 63) == _lib.PSG_ERR_SIZE
    assert L.psg_freq_table_assign(ctx, 0, ptr(t), 65) == _lib.PSG_ERR_SIZE
    assert L.psg_freq_table_assign(ctx, 1, ptr(t), 64) == _lib.PSG_ERR_ARG   # no such filter
    t[:64] = np.arange(64) * 3
    assert L.psg_freq_table_assign(ctx, 0, ptr(t), 64) == _lib.PSG_OK
    assert resumed.freq_table().tolist() == t[:64].tolist()
    for wk in (whole, resumed):
        wk.close()
        wk.model.close()


# ----------------------------------------------------------- evaluate_model --
def test_evaluate_model_is_the_reference_loop(tmp_path):
    rng = np.random.default_rng(19)
    ids = np.unique(rng.integers(1, 1 << 62, size=200, dtype=np.uint64))
    lines = []
    for _ in range(300):
        row = np.sort(rng.choice(ids, size=int(rng.integers(1, 12)), replace=False))
        feats = " ".join("%d:%.6g" % (k, v) for k, v in zip(row.tolist(),
                                                            rng.standard_normal(row.size)))
        lines.append(("%d %s" % (rng.choice([-1, 1]), feats)).rstrip() + "\n")
    text = "".join(lines).encode()
    known = rng.permutation(ids)[:150]
    a, b = str(tmp_path / "part-0"), str(tmp_path / "part-1")
    with open(a, "w") as f:
        for k in known[:100].tolist():
            f.write("%d\t%g\n" % (k, rng.standard_normal()))
    with open(b, "w") as f:
        for k in known[60:].tolist():    # 40 keys of part-0 again: the later file wins
            f.write("%d\t%g\n" % (k, rng.standard_normal()))
        f.write("%d\t%g\n" % (1 << 63, 2.0))   # a key no example holds
    for real in (np.float32, np.float64):
        auc, y, xw = evaluate_model([a, b], text, "libsvm", max_rows=64, real=real)
        mk, mw = read_model_text([a, b], real=real)
        weight = dict(zip(mk.tolist(), mw.tolist()))
        offset, index, value, labels, r = parse_text_host(text, "libsvm")
        assert r.rows == 300 and r.bad_line == -1
        os_, idx, val = offset.tolist(), index.tolist(), value.tolist()
        want = []
        for i in range(300):             # model_evaluation.h:48-57, in double
            re = 0.0
            for j in range(os_[i], os_[i + 1]):
                if idx[j] in weight:
                    re += weight[idx[j]] * val[j]
            want.append(re)
        assert np.array_equal(R.bits(y), R.bits(labels))
        assert np.array_equal(R.bits(xw), R.bits(want)), real
        assert np.count_nonzero(xw) > 200
        assert auc == A.scalar_exact(labels, want)
