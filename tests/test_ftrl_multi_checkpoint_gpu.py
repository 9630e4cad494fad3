"""GPU: checkpoint and restore of the multi-model FTRL (psg_ftrlm_export_state,
psg_ftrlm_import, psg_ftrlm_import_weights; FTRLMultiModel.state / restore /
save / load, FTRLMultiWorker.save / load, evaluate_models).  The reference is
tests/ftrl_ref.py's VectorFTRL, one per column; everything is compared by bits."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import ftrl_ref
from parameter_server_amd import _lib
from parameter_server_amd.ftrl import FTRLMultiModel
from parameter_server_amd.worker import FTRLMultiWorker, evaluate_model, evaluate_models

pytestmark = pytest.mark.gpu

MS = (1, 3, 8, 32)  # G = 1, 4 with an idle lane, 8, 32
U64MAX = (1 << 64) - 1
DTYPES = (np.uint64, np.uint64, np.uint64, np.float64, np.float64)


def ptr(a):
    return a.ctypes.data


def sweep(m):
    """m settings that differ; column m // 2 thresholds many weights to -0.0."""
    p = [dict(alpha=0.5 + 0.1 * j, beta=1.0 + 0.05 * j, lambda1=0.1 * j, lambda2=0.1 + 0.01 * j)
         for j in range(m)]
    p[m // 2]["lambda1"] = 4.0
    return p


def same(got, want, what=""):
    for name, g, w in zip(("keys", "pos", "neg", "w", "z"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


@functools.lru_cache(maxsize=None)
def trained(m, n):
    """(params, three overlapping messages over n keys, the image of the m
    VectorFTRL models after them).  The keys hold 0 first and 2^64 - 1 next;
    every fifth gradient row is zeros, so those keys' first weights are -0.0."""
    rng = np.random.default_rng(1000 * m + n)
    ends = np.array([0, U64MAX][:n], np.uint64)
    keys = np.unique(np.concatenate([rng.integers(1, 1 << 63, size=max(n - 2, 0), dtype=np.uint64),
                                     ends]))
    assert keys.size == n
    msgs = []
    for k in (keys[:(2 * n + 2) // 3], keys[n // 3:], keys[::2]):
        grad = 2.0 * rng.standard_normal((k.size, m))
        grad[::5] = 0.0
        msgs.append((k, rng.integers(0, 6, size=k.size).astype(np.uint32),
                     rng.integers(0, 6, size=k.size).astype(np.uint32), grad))
    params = sweep(m)
    refs = [ftrl_ref.VectorFTRL(**p) for p in params]
    for k, pos, neg, grad in msgs:
        for j, ref in enumerate(refs):
            ref.push(k, pos, neg, grad[:, j])
    r0 = refs[0]
    image = (r0.keys, r0.pos, r0.neg,
             np.ascontiguousarray(np.stack([r.w for r in refs], axis=1)).reshape(n, m),
             np.ascontiguousarray(np.stack([r.z for r in refs], axis=1)).reshape(n, m))
    return params, msgs, image, [r.nnz for r in refs]


def model_of(m, n, hint):
    params, msgs, _, _ = trained(m, n)
    model = FTRLMultiModel(params, capacity_hint=hint)
    for msg in msgs:
        model.push(*msg)
    return model


def random_image(rng, keys, m):
    """Entries with counts past 2^32, -0.0 and +0.0 weights and a NaN payload in z."""
    n = keys.size
    w = rng.standard_normal((n, m))
    w[rng.random((n, m)) < 0.3] = -0.0
    w[rng.random((n, m)) < 0.1] = 0.0
    z = rng.standard_normal((n, m))
    z.view(np.uint64)[0, 0] = 0x7FF800000000BEEF
    return (keys, rng.integers(0, 1 << 40, size=n, dtype=np.uint64),
            rng.integers(0, 1 << 40, size=n, dtype=np.uint64), w, z)


def upsert(old, new):
    """The image after `new` is imported over `old`."""
    keys = np.union1d(old[0], new[0])
    out = [keys] + [np.zeros((keys.size,) + a.shape[1:], a.dtype) for a in old[1:]]
    for img in (old, new):
        at = np.searchsorted(keys, img[0])
        for o, a in zip(out[1:], img[1:]):
            o[at] = a
    return tuple(out)


def check_counts_and_norms(model, image):
    entries, nnz, norm1, norm2 = model.status()
    w = image[3]
    assert entries == image[0].size
    assert nnz.tolist() == np.count_nonzero(w != 0, axis=0).tolist()  # -0.0 is zero, NaN is not
    for j in range(w.shape[1]):
        if not np.isnan(w[:, j]).any():
            s1, s2 = math.fsum(np.abs(w[:, j])), math.fsum(w[:, j] * w[:, j])
            assert abs(norm1[j] - s1) <= entries * 2.0 ** -53 * s1
            assert abs(norm2[j] - s2) <= entries * 2.0 ** -53 * s2


# ---------------------------------------------------------------- export --
@pytest.mark.parametrize("n", (0, 1, 2, 257, 5000))
@pytest.mark.parametrize("m", MS)
def test_export_is_the_model_by_key(m, n):
    _, _, image, nnz = trained(m, n)
    a, b = model_of(m, n, 64), model_of(m, n, 1 << 15)  # a's index grows on the way
    got = a.state()
    same(got, image, "the image of the m models")
    same(b.state(), got, "another capacity hint")
    if n >= 257:
        assert np.any((image[3] == 0) & np.signbit(image[3])) and np.any(image[3] != 0)
    assert a.status()[0] == n and a.status()[1].tolist() == nnz
    a.close()
    b.close()


@pytest.mark.parametrize("m", MS)
def test_ranges_and_errors(m):
    n = 257
    _, _, image, _ = trained(m, n)
    model = model_of(m, n, 64)
    k = image[0]
    for lo, hi in ((int(k[3]), int(k[200])), (int(k[3]) + 1, int(k[200]) - 1),
                   (int(k[5]) + 1, int(k[6]) - 1), (0, 0), (U64MAX, U64MAX), (0, U64MAX),
                   (1, U64MAX - 1)):
        keep = (k >= np.uint64(lo)) & (k <= np.uint64(hi))
        same(model.state((lo, hi)), tuple(a[keep] for a in image), (lo, hi))
    L, h = model._L, model._h
    cnt = C.c_size_t()
    bad = (C.c_uint64 * 2)(5, 4)
    assert L.psg_ftrlm_export_state(h, bad, None, None, None, None, None, 0, C.byref(cnt)) == \
        _lib.PSG_ERR_ARG
    out = [np.full(n if i < 3 else (n, m), 7, dt) for i, dt in enumerate(DTYPES)]
    assert L.psg_ftrlm_export_state(h, None, *[ptr(a) for a in out], n - 1, C.byref(cnt)) == \
        _lib.PSG_ERR_SIZE
    assert cnt.value == n and all((a == 7).all() for a in out)
    args = [ptr(np.ascontiguousarray(a)) for a in image]
    for i in range(5):
        holed = args[:i] + [None] + args[i + 1:]
        assert L.psg_ftrlm_import(h, holed[0], n, *holed[1:]) == _lib.PSG_ERR_ARG
    for j in (-1, m):
        assert L.psg_ftrlm_import_weights(h, j, args[0], n, ptr(image[3][:, 0].copy())) == \
            _lib.PSG_ERR_ARG
    same(model.state(), image, "nothing was applied")
    assert not model.frozen
    model.close()


# ---------------------------------------------------------------- import --
@pytest.mark.parametrize("m", MS)
def test_import_is_an_upsert_with_every_bit_kept(m):
    rng = np.random.default_rng(40 + m)
    keys = np.unique(np.concatenate([rng.integers(1, 1 << 63, size=5200, dtype=np.uint64),
                                     np.array([0, U64MAX], np.uint64)]))
    first = random_image(rng, keys[:5000], m)
    model = FTRLMultiModel(sweep(m), capacity_hint=64)  # the table must grow
    model.restore(*first)
    same(model.state(), first, "an import into an empty model")
    check_counts_and_norms(model, first)
    # some keys again (the last one wins) and new ones, key 2^64 - 1 among them; a NaN weight
    again = np.union1d(keys[:5000:3], keys[5000:])
    second = random_image(rng, again, m)
    second[3][1, m - 1] = np.nan
    model.restore(*second)
    want = upsert(first, second)
    same(model.state(), want, "an import over some of the keys")
    check_counts_and_norms(model, want)
    model.close()


def test_an_unsorted_import_applies_nothing_and_is_reported_once():
    m = 3
    _, _, image, _ = trained(m, 257)
    model = model_of(m, 257, 64)
    rng = np.random.default_rng(5)
    bad = list(random_image(rng, image[0].copy(), m))
    bad[0][[10, 11]] = bad[0][[11, 10]]
    model.restore(*bad)
    model.restore_weights(1, bad[0], bad[3][:, 1].copy())
    with pytest.raises(_lib.PSGError) as e:
        model.status()
    assert e.value.status == _lib.PSG_ERR_UNSORTED
    model.status()  # reported once
    same(model.state(), image, "both messages applied nothing")
    model.close()


# ---------------------------------------------------------------- worker --
def minibatches(seed=31, nbatch=4, rows=300, ids=2000):
    rng = np.random.default_rng(seed)
    table = np.unique(rng.integers(1, U64MAX, size=ids + 50, dtype=np.uint64))[:ids]
    out = []
    for _ in range(nbatch):
        offset = np.concatenate([[0], np.cumsum(rng.integers(1, 13, size=rows))]).astype(np.uint64)
        index = table[rng.zipf(1.3, size=int(offset[-1])) % ids]
        out.append((offset, index, 0.25 * rng.standard_normal(index.size),
                    rng.choice([-1.0, 1.0], size=rows)))
    return out


@pytest.mark.parametrize("freq", (0, 2))
def test_restored_equals_uninterrupted(freq, tmp_path):
    m = 3
    batches = minibatches()

    def worker():
        return FTRLMultiWorker(FTRLMultiModel(sweep(m), capacity_hint=64), tail_feature_freq=freq,
                               countmin_n=1 << 12, countmin_k=2)

    whole, first = worker(), worker()
    for b in batches:
        whole.step(*b)
    for b in batches[:2]:
        first.step(*b)
    path = str(tmp_path / "sweep.ckpt")
    first.save(path)
    mid = first.model.state()
    first.close()
    first.model.close()
    alone = FTRLMultiModel.load(path)
    assert alone.m == m and alone.params == sweep(m) and not alone.frozen
    same(alone.state(), mid, "the model alone")
    alone.close()
    resumed = FTRLMultiWorker.load(path)
    for b in batches[2:]:
        resumed.step(*b)
    same(resumed.model.state(), whole.model.state(), "after four minibatches")
    assert whole.model.state()[0].size > 30
    assert resumed.objv.tobytes() == whole.objv.tobytes() and (whole.objv > 0).all()
    assert resumed.num_ex == whole.num_ex == 1200
    assert resumed.freq == freq
    if freq:  # the filter travels only when it is on
        assert (resumed.countmin_n, resumed.countmin_k) == (1 << 12, 2)
        assert resumed.freq_table().tobytes() == whole.freq_table().tobytes()
    for wk in (whole, resumed):
        wk.close()
        wk.model.close()


# ---------------------------------------------------------------- frozen --
def libsvm_text(rng, ids, lines):
    out = []
    for _ in range(lines):
        row = np.sort(rng.choice(ids, size=int(rng.integers(1, 12)), replace=False))
        feats = " ".join("%d:%.6g" % kv for kv in zip(row.tolist(), rng.standard_normal(row.size)))
        out.append("%d %s\n" % (rng.choice([-1, 1]), feats))
    return "".join(out).encode()


def test_a_saved_sweep_is_scored_as_its_models_are_one_by_one(tmp_path):
    m = 3
    rng = np.random.default_rng(77)
    ids = np.unique(rng.integers(1, 1 << 62, size=200, dtype=np.uint64))
    params = [dict(alpha=0.5, beta=1.0, lambda1=l1, lambda2=0.1) for l1 in (0.0, 0.3, 0.05)]
    model = FTRLMultiModel(params, capacity_hint=64)
    wk = FTRLMultiWorker(model)
    train = libsvm_text(rng, ids, 300)
    at = 0
    for _ in range(2):
        at += wk.step_text(train[at:], "libsvm", 150)[2]
    paths = [[str(tmp_path / ("model-%d" % j))] for j in range(m)]
    for j in range(m):
        model.writeToFile(j, paths[j][0])
    shared = model.export(0)[0][:40]
    before = model.lookup(shared)
    wk.close()

    text = libsvm_text(rng, ids, 500)
    auc, y, xw = evaluate_models(paths, text, "libsvm", max_rows=200)
    assert xw.shape == (500, m) and np.count_nonzero(xw[:, 0]) > 250
    for j in range(m):
        a1, y1, xw1 = evaluate_model(paths[j], text, "libsvm", max_rows=200)
        assert y.tobytes() == y1.tobytes()
        assert np.ascontiguousarray(xw[:, j]).tobytes() == xw1.tobytes(), j
        assert np.float64(auc[j]).tobytes() == np.float64(a1).tobytes(), j

    # column 1 alone over a trained model: the other columns of shared keys stay
    fresh_key = np.array([U64MAX], np.uint64)
    new_w = rng.standard_normal(shared.size + 1)
    assert not model.frozen
    model.restore_weights(1, np.concatenate([shared, fresh_key]), new_w)
    assert model.frozen
    pos, neg, w, z, found = model.lookup(np.concatenate([shared, fresh_key]))
    assert found.all() and w[:, 1].tobytes() == new_w.tobytes()
    for got, want in zip((pos[:-1], neg[:-1], w[:-1, [0, 2]], z[:-1]),
                         (before[0], before[1], before[2][:, [0, 2]], before[3])):
        assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()
    assert (pos[-1], neg[-1]) == (0, 0) and not w[-1, [0, 2]].any() and not z[-1].any()
    with pytest.raises(_lib.PSGError) as e:
        model.push(shared[:1], [1], [0], np.ones((1, m)))
    assert e.value.status == _lib.PSG_ERR_ARG
    assert model.pull(shared)[:, 1].tobytes() == new_w[:-1].tobytes()
    model.close()
