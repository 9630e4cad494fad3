"""GPU: the direct scorer (psg_ftrl_score_dev, psg_ftrlm_score_dev; FTRLWorker /
FTRLMultiWorker.score, evaluate_model(s)(score="direct")) against a Python dict
and a sequential loop per row that skips absent keys, bit for bit."""
import numpy as np
import pytest

from parameter_server_amd import _lib
from parameter_server_amd.ftrl import FTRLModel, FTRLMultiModel, format_weight
from parameter_server_amd.worker import (FTRLMultiWorker, FTRLWorker, Minibatch, evaluate_model,
                                         evaluate_models, score_tile)

pytestmark = pytest.mark.gpu

PARAM = dict(alpha=1.0, beta=1.0, lambda1=0.0, lambda2=0.0)


def ref_score(table, offset, index, value, real):
    """model_evaluation.h:48-57 with Real = `real`: table maps key -> w[m]."""
    m = len(next(iter(table.values())))
    out = np.zeros((offset.size - 1, m), np.float64)
    with np.errstate(all="ignore"):
        for i in range(offset.size - 1):
            re = np.zeros(m, real)
            for j in range(int(offset[i]), int(offset[i + 1])):
                w = table.get(int(index[j]))
                if w is not None:
                    re = re + (w.astype(real) * real(value[j]) if value is not None
                               else w.astype(real))
            out[i] = re.astype(np.float64)
    return out


@pytest.mark.parametrize("binary", (True, False), ids=("binary", "valued"))
@pytest.mark.parametrize("real", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("m", (0, 1, 3, 32), ids=("scalar", "m1", "m3", "m32"))
def test_score_is_the_reference_loop(m, real, binary):
    T, cols = score_tile(m, real), max(m, 1)
    rng = np.random.default_rng(100 * m + (real is np.float32) + 2 * binary)
    # ends on the edge T | ten empties on it | in tile 1 | a short row over 2T | 2T + 5 over 3T and 4T |
    # one-entry rows | a row over 5T | a row of 51 over 6T that leaves the last tile one entry |
    # empties all round; every length is positive down to a tile of 64
    lens = [0, 1, T - 1] + [0] * 10 + [10, T - 20, 25, 2 * T + 5, 1, 1, 1, 0, 2 * T - 73, 51, 0]
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nnz = int(offset[-1])
    assert nnz == 6 * T + 1 and min(lens) == 0 and T >= 64
    # 3000 keys at half load: ~6 % of the buckets hold more than three keys, so
    # some sit past their first bucket; a quarter of the sweep's slots collide
    zero_present = real is np.float64
    present = np.unique(rng.integers(1, 1 << 63, size=3000, dtype=np.uint64))
    absent = present[::3] + np.uint64(1)
    absent = absent[~np.isin(absent, present)]
    if zero_present:
        present = np.concatenate([[np.uint64(0)], present])
    w = rng.standard_normal((present.size, cols))
    index = np.where(rng.random(nnz) < 0.7, rng.choice(present, nnz), rng.choice(absent, nnz))
    value = rng.standard_normal(nnz)
    # the row of 10 at T: an order-dependent sum, a repeated key, key 0, both zero weights
    big, at = (1e16 if real is np.float64 else 1e8), T
    sp = np.arange(10, 20)  # rows of `present` (sorted: 0 first if there) with chosen weights
    index[at:at + 10] = [present[s] for s in (10, 11, 12, 13, 14, 14, 15, 16, 17, 18)]
    index[at + 9], index[0], index[3 * T] = 0, 0, 0
    seq = np.array([big, 1.0, -big, 1.0])
    w[sp[:4]] = seq[:, None] if binary else 1.0
    value[at:at + 4] = 1.0 if binary else seq
    w[sp[5]], w[sp[6]] = 0.0, -0.0
    value[at + 7] = -0.0
    index[at + 8], value[at + 8] = absent[0], np.inf  # skipped: the sum stays finite
    index[2 * T - 3:2 * T + 3] = present[40]  # one key on both sides of an edge
    y = rng.choice([-1.0, 1.0], size=offset.size - 1)
    val = None if binary else value
    want = ref_score(dict(zip(present.tolist(), w)), offset, index, val, real)
    assert np.isfinite(want).all() and lens[13] == 10 and want[13, 0] != 0

    cnt = np.zeros(present.size, np.uint64)
    if m == 0:
        model = FTRLModel(capacity_hint=64)
        model.restore(present, cnt, cnt, w[:, 0], w[:, 0])
        wk = FTRLWorker(model)
    else:
        model = FTRLMultiModel([PARAM] * m, capacity_hint=64)
        model.restore(present, cnt, cnt, w, w)
        wk = FTRLMultiWorker(model)
    before = (model.status()[0], [a.tobytes() for a in model.state()])
    if m == 0:
        wk.score(offset, index, val, y, real=real)
        got = wk.mb.read("xw")[:, None]
    else:
        got = wk.score(offset, index, val, y, real=real)
    assert got.shape == want.shape
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    assert bad.size == 0, (bad[:8], got[bad[:3]], want[bad[:3]])
    # the model is untouched by scoring a minibatch with absent keys
    assert (model.status()[0], [a.tobytes() for a in model.state()]) == before

    # with finite values the predict path gives the same bits (F64 only: it has no float form)
    if real is np.float64:
        if not binary:
            value[at + 8] = 2.5
        if m == 0:
            wk.predict(offset, index, val, y)
            old = wk.mb.read("xw")[:, None]
            wk.score(offset, index, val, y)
            new = wk.mb.read("xw")[:, None]
        else:
            old, new = wk.predict(offset, index, val, y), wk.score(offset, index, val, y)
        assert old.tobytes() == new.tobytes()
        value[at + 8] = np.inf
    wk.close()
    model.close()
    # column j of the sweep is the scalar call on a scalar model given column j's weights
    for j in ((0, m - 1) if m > 1 else ()):
        one = FTRLModel(capacity_hint=64)
        one.restore(present, cnt, cnt, w[:, j], w[:, j])
        wj = FTRLWorker(one)
        wj.score(offset, index, val, y, real=real)
        assert wj.mb.read("xw").tobytes() == np.ascontiguousarray(got[:, j]).tobytes(), j
        wj.close()
        one.close()


@pytest.mark.parametrize("m", (0, 3), ids=("scalar", "m3"))
def test_no_rows_and_no_entries(m):
    model = FTRLModel() if m == 0 else FTRLMultiModel([PARAM] * m)
    keys = np.array([5], np.uint64)
    one, cnt = np.ones((1, max(m, 1))), np.zeros(1, np.uint64)
    model.restore(keys, cnt, cnt, one[:, 0] if m == 0 else one, one[:, 0] if m == 0 else one)
    wk = (FTRLWorker if m == 0 else FTRLMultiWorker)(model)
    none = np.zeros(0, np.uint64)
    for rows in (0, 4):
        got = wk.score(np.zeros(rows + 1, np.uint64), none, None, np.ones(rows))
        got = wk.mb.read("xw") if m == 0 else got
        assert got.size == rows * max(m, 1) and not got.view(np.uint64).any()
    wk.close()
    model.close()


def test_a_saved_model_is_scored_in_float(tmp_path):
    rng = np.random.default_rng(5)
    ids = np.unique(rng.integers(1, 1 << 62, size=300, dtype=np.uint64))
    m, lines = 3, []
    w = rng.standard_normal((ids.size, m))
    paths = [[str(tmp_path / ("model-%d" % j))] for j in range(m)]
    for j in range(m):  # every third key is missing from the files
        with open(paths[j][0], "w") as f:
            f.writelines("%d\t%s\n" % (k, format_weight(x)) for k, x in zip(ids[::3], w[::3, j]))
            f.writelines("%d\t%s\n" % (k, format_weight(x)) for k, x in zip(ids[1::3], w[1::3, j]))
    for _ in range(500):
        row = np.sort(rng.choice(ids, size=int(rng.integers(1, 12)), replace=False))
        lines.append("%d %s\n" % (rng.choice([-1, 1]), " ".join(
            "%d:%.6g" % kv for kv in zip(row.tolist(), rng.standard_normal(row.size)))))
    text = "".join(lines).encode()
    auc, y, xw = evaluate_models(paths, text, "libsvm", max_rows=200, score="direct")
    assert xw.shape == (500, m)
    # the float reference loop over what the files and the text hold
    holder = FTRLModel()
    mb = Minibatch(holder._h)
    mb.load_text(text, "libsvm")
    offset, index, value = mb.read("offset"), mb.read("index"), mb.read("value")
    mb.close()
    holder.close()
    for j in range(m):
        frozen = FTRLModel()
        frozen.readFromFile(paths[j], real=np.float32)
        assert frozen.frozen
        before = [a.tobytes() for a in frozen.state()]
        wk = FTRLWorker(frozen)
        wk.score(offset, index, value, y, real=np.float32)
        assert [a.tobytes() for a in frozen.state()] == before and frozen.frozen
        table = {int(k): np.array([x]) for k, x in zip(*frozen.state()[0::3])}
        want = ref_score(table, offset, index, value, np.float32)[:, 0]
        assert wk.mb.read("xw").tobytes() == want.tobytes()
        a1, y1, xw1 = evaluate_model(paths[j], text, "libsvm", max_rows=200, score="direct",
                                     real=np.float32)
        assert xw1.tobytes() == want.tobytes() and y1.tobytes() == y.tobytes()
        assert np.ascontiguousarray(xw[:, j]).tobytes() == xw1.tobytes(), j
        assert np.float64(auc[j]).tobytes() == np.float64(a1).tobytes(), j
        wk.close()
        frozen.close()


def test_errors():
    L, ARG = _lib.lib(), _lib.PSG_ERR_ARG
    scalar, multi = FTRLModel(), FTRLMultiModel([PARAM] * 2)
    hs, hm = scalar._model(), multi._model()
    mbs, mbm = Minibatch(hs), Minibatch(hm)
    out = mbs.scratch(0, 64)
    outm = mbm.scratch(0, 64)
    assert L.psg_ftrl_score_dev(hs, mbs._h, _lib.PSG_SCORE_F64, None, None) == ARG  # not loaded
    assert L.psg_ftrlm_score_dev(hm, mbm._h, _lib.PSG_SCORE_F64, outm, None) == ARG
    off, idx, y = np.array([0, 1], np.uint64), np.array([7], np.uint64), np.ones(1)
    mbs.load(off, idx, None, y)
    mbm.load(off, idx, None, y)
    assert L.psg_ftrl_score_dev(hs, mbs._h, 2, None, None) == ARG  # unknown real
    assert L.psg_ftrlm_score_dev(hm, mbm._h, -1, outm, None) == ARG
    assert L.psg_ftrlm_score_dev(hs, mbs._h, _lib.PSG_SCORE_F64, out, None) == ARG  # no sweep
    assert L.psg_ftrl_score_dev(hm, mbm._h, _lib.PSG_SCORE_F64, None, None) == ARG  # no scalar
    assert L.psg_ftrl_score_dev(hs, mbs._h, _lib.PSG_SCORE_F64, None, None) == _lib.PSG_OK
    assert L.psg_ftrlm_score_dev(hm, mbm._h, _lib.PSG_SCORE_F32, outm, None) == _lib.PSG_OK
    assert not mbs.read("xw").view(np.uint64).any()  # key 7 is absent
    for h in (mbs, mbm, scalar, multi):
        h.close()
