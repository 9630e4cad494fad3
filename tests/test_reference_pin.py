"""The CPU restatements against the reference's own code (no GPU).

The chain behind every bit-exactness claim is GPU kernel == CPU restatement
== reference.  This file tests the second link:

recorded  tests/golden/reference_pin/*.npz hold what the reference's own
          match / oldMatch / sliceKeyOrderedMsg / evenDivide, FTRLModel and
          FreqencyFilter (compiled in place, oracle/ref_*_shim.cc) returned
          on the fixed inputs of tests/pin_cases.py, written by
          tools/record_reference.py.  Every restatement must reproduce them
          bit for bit.  These tests always run.
live      where oracle/_ref holds the three libraries (the reference tree was
          present when `make -C oracle` ran), seeded cases beyond the
          fixtures run the reference's code and the restatement side by side.
          Elsewhere they skip, naming the library.
"""
import math
import os

import numpy as np
import pytest

import ftrl_ref as F
import oracle_py as O
import pin_cases as P
import ref_py as R
from test_freq_filter import py_insert, py_query


def need(which):
    if not R.available(which):
        pytest.skip("oracle/_ref/%s not built (reference tree absent)" % R.LIBS[which])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(P.fbits(a), P.fbits(b))


# ------------------------------------------------------------------- helpers
def test_unmix64_inverts_fmix64():
    h = P.splitmix64(77, 10_000)
    assert np.array_equal(P.fmix64(P.unmix64(h)), h)
    assert np.array_equal(P.unmix64(P.fmix64(h)), h)
    edge = np.array([0, 1, P.U64, 1 << 63, P.LOW24], np.uint64)
    assert np.array_equal(P.fmix64(P.unmix64(edge)), edge)
    assert int(P.fmix64(np.array([1], np.uint64))[0]) == 0xb456bcfc34c2cb2c  # MurmurHash3 fmix64(1)


def test_fixtures_are_small_and_say_their_source():
    names = sorted(os.listdir(P.GOLDEN))
    assert names == ["countmin.npz", "even_divide.npz", "fold_F1_r0.npz", "fold_F2_r0.npz",
                     "fold_F2_r1.npz", "fold_F3_r0.npz", "ftrl_parity.npz", "ftrl_steep.npz"]
    for n in names:
        assert os.path.getsize(os.path.join(P.GOLDEN, n)) <= 128 * 1024, n
        meta, arrays = P.load_fixture(n[:-4])
        assert "compiled in place" in meta["source"]
        for a in arrays.values():
            assert a.dtype.kind in "iub"  # bit patterns and counts: data only


# ---------------------------------------------------------------- evenDivide
def test_even_divide_recorded():
    from parameter_server_amd.kv_vector import shard_bounds
    meta, arrays = P.load_fixture("even_divide")
    b, e = meta["range_all"]
    assert (b, e) == (0, P.U64)
    for n in P.EVEN_DIVIDE_N:
        want = arrays["n%d" % n]
        got = np.array([O.even_divide(b, e, n, i) for i in range(n)], np.uint64)
        assert np.array_equal(got, want), n
        sb = shard_bounds(n)
        assert np.array_equal(sb[:-1], want[:, 0]) and np.array_equal(sb[1:], want[:, 1]), n


# ---------------------------------------------------------------------- fold
FOLD_FIXTURES = [("F1", 0), ("F2", 0), ("F2", 1), ("F3", 0)]
_fold_cache = {}


def fold(name):
    if name not in _fold_cache:
        _fold_cache[name] = P.fold_case(name)
    return _fold_cache[name]


def check_slice(D, kb, ke, sep, begin, end, valid):
    pos, ovalid = O.slice_key_ordered(D, kb, ke, sep)
    assert np.array_equal(ovalid, valid)
    ok = valid == 1
    assert np.array_equal(pos[:-1][ok].astype(np.int64), begin[ok])
    assert np.array_equal(pos[1:][ok].astype(np.int64), end[ok])


@pytest.mark.parametrize("name,r", FOLD_FIXTURES)
def test_fold_recorded(name, r):
    c = fold(name)
    meta, fx = P.load_fixture(c.fixture(r))
    assert meta["input_sha256"] == c.digest()
    kb, ke = meta["key_range"]
    pushes = c.sliced(r)
    assert len(pushes) == meta["npush"] and (c.dtype.name, c.m) == (meta["dtype"], meta["m"])
    lo, hi = meta["positions"]
    want = {mode: [fx["%s%d" % (mode, i)] for i in range(c.m)] for mode in ("serial", "parallel")}
    runs = [("serial", O.aggregate(c.D, kb, ke, pushes, False, 1, c.dtype)),
            ("serial", O.aggregate_scatter(c.D, kb, ke, pushes, c.dtype, parallel=False))]
    for t in (1, 2, 4):
        runs.append(("parallel", O.aggregate(c.D, kb, ke, pushes, True, t, c.dtype)))
    runs.append(("parallel", O.aggregate_scatter(c.D, kb, ke, pushes, c.dtype, parallel=True)))
    for mode, (rc, glo, ghi, got, mt) in runs:
        assert rc == 0 and (glo, ghi) == (lo, hi)
        assert np.array_equal(mt, fx["matched"])
        for i in range(c.m):
            assert np.array_equal(P.fbits(got[i]), want[mode][i]), (mode, i)
    out, gm = O.gather(c.D, c.W, c.R, c.dtype)
    assert gm == meta["gather_matched"] and np.array_equal(P.fbits(out), fx["gather"])
    check_slice(c.D, kb, ke, fx["slice_sep"], fx["slice_begin"], fx["slice_end"], fx["slice_valid"])
    _, ed = P.load_fixture("even_divide")
    assert np.array_equal(fx["slice_sep"], np.concatenate([ed["n8"][:, 0], ed["n8"][-1:, 1]]))


# ---------------------------------------------------------------------- FTRL
_ftrl_cache = []


def ftrl():
    if not _ftrl_cache:
        _ftrl_cache.append(P.ftrl_case())
    return _ftrl_cache[0]


@pytest.mark.parametrize("cls", [F.ScalarFTRL, F.VectorFTRL])
@pytest.mark.parametrize("pname", sorted(P.FTRL_PARAMS))
def test_ftrl_recorded(pname, cls):
    c = ftrl()
    meta, fx = P.load_fixture("ftrl_" + pname)
    assert meta["input_sha256"] == c.digest()
    param = P.FTRL_PARAMS[pname]
    assert meta["param"] == param
    m = cls(**param)
    for msg, want in zip(c.msgs, meta["after"]):
        m.push(*msg)
        assert (m.entries, m.nnz) == (want["size"], want["nnz"])
        assert P.entry_digest(*m.lookup(c.keys)) == want["entries_sha256"]
    pos, neg, w, z, found = m.lookup(c.keys)
    assert np.array_equal(pos, fx["pos"]) and np.array_equal(neg, fx["neg"])
    assert np.array_equal(F.bits(w), fx["w"]) and np.array_equal(F.bits(z), fx["z"])
    assert np.array_equal(found, fx["found"])
    text = fx["dump_text"].tobytes().decode()
    assert F.dump_text(m, c.keys) == text
    k, wn = F.nonzero(m, c.keys)
    assert len(text.splitlines()) == k.size == m.nnz and np.all(wn != 0)
    assert [int(ln.split("\t")[0]) for ln in text.splitlines()] == k.tolist()
    assert np.array_equal(F.bits(F.pull(m, c.request)), fx["pull"])
    # a pull inserts in the reference: every absent key asked for is an entry
    assert meta["size_after_pull"] == m.entries + int((~np.isin(np.unique(c.request), c.keys[found == 1])).sum())


@pytest.mark.parametrize("pname", sorted(P.FTRL_PARAMS))
def test_ftrl_objv_within_the_stated_bound(pname):
    """norm1 / norm2 are a defined deviation (a reduction, not the
    reference's running sums), so objv is compared with the exact value, not
    bit for bit.  With the two infinite-gradient keys the reference's norms
    are inf - inf = NaN; the bound is checked on the run without them.  The
    weights are the restatement's, which test_ftrl_recorded holds to the
    reference's bit for bit; the product's own objv is held to the same
    interval in tests/test_ftrl_gpu.py."""
    c = ftrl()
    meta, _ = P.load_fixture("ftrl_" + pname)
    param = P.FTRL_PARAMS[pname]
    assert math.isnan(np.array([int(meta["objv_bits"], 16)], np.uint64).view(np.float64)[0])
    m = F.VectorFTRL(**param)
    for msg in c.finite_msgs():
        m.push(*msg)
    assert m.nnz == meta["finite_nnz"]
    w = m.lookup(c.keys)[2]
    assert np.isfinite(w).all()
    w = w.tolist()
    lo, hi = P.objv_interval(w, m.entries, param["lambda1"], param["lambda2"])
    ref = float(np.array([int(meta["finite_objv_bits"], 16)], np.uint64).view(np.float64)[0])
    print("objv %s: reference %r, interval [%r, %r]" % (pname, ref, lo, hi))
    assert math.isfinite(ref) and lo <= ref <= hi


# ------------------------------------------------------------------ CountMin
def kept_keys(query, packed, info):
    mask = np.unpackbits(packed)[: query.size].astype(bool)
    kept = query[mask]
    assert kept.size == info["n"] and P.sha256([kept]) == info["sha256"]
    return kept


@pytest.mark.parametrize("n,k", P.CM_SHAPES)
def test_countmin_recorded(n, k):
    meta, fx = P.load_fixture("countmin")
    tag = "n%d_k%d" % (n, k)
    info = meta["cases"][tag]
    c = P.cm_case(n, k)
    assert info["input_sha256"] == c.digest()
    assert (info["empty_before_resize"], info["empty_after_resize"], info["empty_after_clear"]) == \
        (True, False, True)
    t, nn, kk = O.cm_resize(n, k)
    assert (nn, kk) == (info["n_"], info["k_"])
    tp = [0] * nn  # the pure-Python form's table
    for keys, counts in c.batches:
        O.cm_insert(t, nn, kk, keys, counts)
        py_insert(tp, nn, kk, keys.tolist(), counts.tolist())
    assert np.array_equal(t, fx[tag + "_table"])
    assert np.array_equal(np.array(tp, np.uint8), fx[tag + "_table"])
    for freq in P.CM_FREQS:
        want = kept_keys(c.query, fx["%s_kept%d" % (tag, freq)], info["kept"][str(freq)])
        assert np.array_equal(O.ff_query(t, nn, kk, c.query, freq), want)
        assert np.array_equal(py_query(tp, nn, kk, c.query.tolist(), freq), want)


# ---------------------------------------------------------------------- live
@pytest.mark.parametrize("seed", range(8))
def test_live_fold(seed):
    need("match")
    c = P.random_fold_case(seed)
    kb, ke = c.ranges[0]
    pushes = c.sliced(0)
    assert pushes
    for parallel in (False, True):
        for t in ((1,) if not parallel else (1, 2, 4)):
            want = R.aggregate(c.D, kb, ke, pushes, parallel, t, c.dtype)
            got = O.aggregate(c.D, kb, ke, pushes, parallel, t, c.dtype)
            sc = O.aggregate_scatter(c.D, kb, ke, pushes, c.dtype, parallel=parallel)
            for other in (got, sc):
                assert other[:3] == want[:3] and np.array_equal(other[4], want[4])
                assert all(same(a, b) for a, b in zip(other[3], want[3]))
    # oldMatch itself over the key range, then match over a position
    # sub-range, ASSIGN then ADD
    lo, hi = O.find_range(c.D, kb, ke)
    for k, vs in pushes[:4]:
        want = R.old_match(c.D, k, vs[-1], kb, ke, c.dtype)
        got = O.old_match(c.D, k, vs[-1], kb, ke, c.dtype)
        assert got[:2] == want[:2] == (lo, hi) and got[3] == want[3] == k.size
        assert same(got[2], want[2])
    if hi - lo >= 8:
        lo2, hi2 = lo + (hi - lo) // 3, hi - (hi - lo) // 5
        k, vs = max(pushes, key=lambda p: p[0].size)
        for t in (1, 2, 4):
            dst = P.scaled(P.splitmix64(seed, hi2 - lo2), c.dtype)
            for add in (0, 1):
                want, wm = R.match(c.D, lo2, hi2, dst, k, vs[0], add, t, c.dtype)
                got, mt = O.match(c.D, lo2, hi2, dst, k, vs[0], add, t, c.dtype)
                assert mt == wm and same(got, want)
                dst = want
    out, gm = R.gather(c.D, c.W, c.R, c.dtype)
    got, om = O.gather(c.D, c.W, c.R, c.dtype)
    assert gm == om and same(got, out)
    n = 1 + seed
    sep = np.array([O.even_divide(0, P.U64, n, i)[0] for i in range(n)] + [P.U64], np.uint64)
    for i in range(n):
        assert R.even_divide(0, P.U64, n, i) == O.even_divide(0, P.U64, n, i)
        assert R.even_divide(kb, ke, n, i) == O.even_divide(kb, ke, n, i)
    b, e, vb, valid = R.slice_key_ordered(c.D, kb, ke, sep)
    assert np.array_equal(b, vb)
    check_slice(c.D, kb, ke, sep, b, e, valid)


def test_live_fixtures_reproduce():
    """The committed fold fixtures are what the reference's code gives today."""
    need("match")
    for name, r in FOLD_FIXTURES:
        c = fold(name)
        meta, fx = P.load_fixture(c.fixture(r))
        kb, ke = meta["key_range"]
        for mode, parallel in (("serial", False), ("parallel", True)):
            rc, lo, hi, got, mt = R.aggregate(c.D, kb, ke, c.sliced(r), parallel, 2, c.dtype)
            assert rc == 0 and [lo, hi] == meta["positions"]
            for i in range(c.m):
                assert np.array_equal(P.fbits(got[i]), fx["%s%d" % (mode, i)])


@pytest.mark.parametrize("seed", range(1, 5))
def test_live_ftrl(seed):
    need("ftrl")
    c = P.ftrl_case(seed=seed, nscatter=300 + 100 * seed)
    param = dict(alpha=[1.0, 0.05, 0.5, 2.0][seed - 1], beta=[1.0, 1.0, 0.25, 3.0][seed - 1],
                 lambda1=[1.0, 0.5, 0.0, 2.0][seed - 1], lambda2=[0.1, 0.0, 1.0, 0.5][seed - 1])
    ref, sc, ve = R.RefFTRL(**param), F.ScalarFTRL(**param), F.VectorFTRL(**param)
    for msg in c.msgs:
        for m in (ref, sc, ve):
            m.push(*msg)
        want = ref.lookup(c.keys)
        for m in (sc, ve):
            assert (m.entries, m.nnz) == (ref.entries, ref.nnz)
            assert all(same(a, b) for a, b in zip(m.lookup(c.keys), want))
    text = P.sorted_dump(ref.dump_text())
    pulled = ref.get_value(c.request)
    for m in (sc, ve):
        assert F.dump_text(m, c.keys) == text
        assert same(F.pull(m, c.request), pulled)


@pytest.mark.parametrize("n,k", [(1, 0), (64, 1), (65, 31), (4099, 7), (100000, 2), (2000, 30)])
def test_live_countmin(n, k):
    need("countmin")
    c = P.cm_case(n, k, seed=3)
    f = R.RefFilter()
    assert f.empty()
    f.resize(n, k)
    t, nn, kk = O.cm_resize(n, k)
    for keys, counts in c.batches:
        f.insert_keys(keys, counts)
        O.cm_insert(t, nn, kk, keys, counts)
    rn, rk, table = f.table()
    assert (rn, rk) == (nn, kk) and np.array_equal(table, t)
    for freq in (0, 1, 50, 254):
        assert np.array_equal(f.query_keys(c.query, freq), O.ff_query(t, nn, kk, c.query, freq))
    f.clear()
    assert f.empty()


def test_live_appendix_c_known_answers():
    """tests/golden/known_answers.json's aggregate / gather constants (SURVEY
    Appendix C) are what the reference's compiled match / oldMatch give."""
    need("match")
    import json
    gold = json.load(open(os.path.join(os.path.dirname(P.GOLDEN), "known_answers.json")))
    for name in ("aggregate", "aggregate_subrange"):
        g = gold[name]
        kb, ke = (0, P.U64) if g["key_range"] == "all" else g["key_range"]
        pushes = [(p["keys"], [p["vals"]]) for p in g["pushes"]]
        for dtype in (np.float32, np.float64):
            for parallel, t in ((False, 1), (True, 1), (True, 2)):
                rc, lo, hi, out, mt = R.aggregate(g["D"], kb, ke, pushes, parallel, t, dtype)
                assert rc == 0 and [lo, hi] == g["positions"] and out[0].tolist() == g["A"]
                assert mt.tolist() == g.get("matched", [len(p["keys"]) for p in g["pushes"]])
    g = gold["gather"]
    out, mt = R.gather(g["D"], g["W"], g["R"])
    assert mt == g["matched"] and out.tolist() == g["out"]
    for n, bounds in gold["shards"].items():
        want = [R.even_divide(0, P.U64, int(n), i)[0] for i in range(int(n))] + [P.U64]
        assert [int(b) for b in bounds] == want
