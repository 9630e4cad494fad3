"""The CPU restatements against the reference's own code (no GPU).

The chain behind every bit-exactness claim is GPU kernel == CPU restatement
== reference.  This file tests the second link:

recorded  tests/golden/reference_pin/*.npz hold what the reference's own
          match / oldMatch / sliceKeyOrderedMsg / evenDivide, FTRLModel,
          FreqencyFilter, AUC, Evaluation<double>::auc and Localizer
          (compiled in place, oracle/ref_*_shim.cc) returned
          on the fixed inputs of tests/pin_cases.py, written by
          tools/record_reference.py.  Every restatement must reproduce them
          bit for bit.  These tests always run.
live      where oracle/_ref holds the libraries (the reference tree was
          present when `make -C oracle` ran), seeded cases beyond the
          fixtures run the reference's code and the restatement side by side.
          Elsewhere they skip, naming the library.
"""
import math
import os

import numpy as np
import pytest

import auc_ref as A
import ftrl_ref as F
import oracle_py as O
import pin_cases as P
import ref_py as R
import worker_ref as W
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
    assert names == ["auc.npz", "auc_merge.npz", "countmin.npz", "even_divide.npz",
                     "exact_auc.npz", "fold_F1_r0.npz", "fold_F2_r0.npz", "fold_F2_r1.npz",
                     "fold_F3_r0.npz", "ftrl_parity.npz", "ftrl_steep.npz", "localizer.npz"]
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


# ----------------------------------------------------------------------- AUC
AUC_PARTS = ("tp_key", "tp_count", "fp_key", "fp_count")
_auc_cache = {}


def auc_cases():
    if not _auc_cache:
        _auc_cache.update({c.name: c for c in P.auc_cases()})
    return _auc_cache


def fb(v):
    """A double's bits as the fixtures spell them; every NaN is one value
    (0 / 0 carries no payload worth keeping, and its sign differs by platform)."""
    return "nan" if math.isnan(v) else "%016x" % int(P.fbits(np.array([v], np.float64))[0])


def recorded_double(hexbits):
    return fb(float(np.array([int(hexbits, 16)], np.uint64).view(np.float64)[0]))


def same_aucdata(fx, sha, name, data):
    return all(P.same_output(fx, sha, "%s.%s" % (name, part), a) for part, a in zip(AUC_PARTS, data))


def test_auc_cases_cover_what_they_claim():
    cases = auc_cases()
    assert len(cases) == len(P.pin_sizes()) * len(P.AUC_GOODNESS) + len(P.AUC_GOODNESS)
    assert {1, 10, 1000, 100000, -1000} <= set(P.AUC_GOODNESS)
    assert P.pin_sizes() == (1, P.PIN_TILE - 1, P.PIN_TILE, P.PIN_TILE + 1, 3 * P.PIN_TILE + 5)
    for c in cases.values():
        with np.errstate(all="ignore"):
            prod = c.p * np.float64(c.g)
        undefined = ~(np.abs(prod) < 2.0 ** 63)
        assert undefined.any() == c.name.startswith("undefined"), c.name
        if c.y.size > 100:
            assert {b for b in P.fbits(c.y).tolist()} == {b for b in P.fbits(P.AUC_LABELS).tolist()}
            assert ((prod > -1) & (prod < 0)).any()
            if not c.name.startswith("undefined"):
                assert (P.fbits(c.p) == np.uint64(1 << 63)).any() and (np.abs(prod) == 1e18).sum() == 2
                assert ((np.abs(c.p) < 2.3e-308) & (c.p != 0)).sum() == 4  # the denormals
    # the decimals do what their comment says, at the goodness that shows it
    assert 0.29 * 100 < 29 and 0.57 * 100 < 57 and 0.1 * 10 == 1 == 0.7 * 10 / 7 and 4.35 * 100 < 435
    assert 0.58 * 100 < 58 and 1.15 * 100 < 115 and 16.08 * 100 < 1608 and 0.029 * 1000 == 29


@pytest.mark.parametrize("name", [c.name for c in P.auc_cases()])
def test_auc_compute_recorded(name):
    c = auc_cases()[name]
    meta, fx = P.load_fixture("auc")
    info = meta["cases"][name]
    assert meta["tile"] == P.PIN_TILE and info["input_sha256"] == c.digest()
    for compute in (A.scalar_compute, A.vector_compute):
        data = compute(c.y, c.p, c.g)
        assert (data[0].size, data[2].size) == (info["ntp"], info["nfp"])
        assert same_aucdata(fx, meta["sha256"], name, data), compute.__name__


def test_auc_probe_of_the_issue():
    """0.29 * 100 -> 28, 0.7 * 100 -> 70, -0.005 * 100 -> 0; the restatement's
    rule is held to the recorded cases above, this is the rule by hand."""
    assert [A.scalar_key(p, 100) for p in (0.29, 0.7, -0.005)] == [28, 70, 0]
    assert A.vector_keys(np.array([0.29, 0.7, -0.005]), 100).tolist() == [28, 70, 0]


def test_auc_undefined_conversions_recorded():
    """include/psg.h: a product that is NaN or of magnitude >= 2^63 "gets the
    key INT64_MIN, which is what the reference's x86-64 build produces".  The
    fixture holds what the reference's compiled compute returned for each such
    prediction on its own."""
    _, fx = P.load_fixture("auc")
    for g in P.AUC_GOODNESS:
        want = fx["undefined_g%d.single_keys" % g]
        bad = P.auc_undefined(g)
        assert want.size == bad.size and (want == A.INT64_MIN).all()
        assert [A.scalar_key(p, g) for p in bad.tolist()] == want.tolist()
        assert np.array_equal(A.vector_keys(bad, g), want)


MERGE_NAMES = sorted(P.auc_merge_sequences())
# sequences in which a side holds zero counts only: the reference's map is not
# empty() there and evaluate divides 0 by 0, the product has dropped the
# entries and returns .5 (include/psg.h, defined deviation)
ZERO_ONLY = {"zero_only_negatives", "zero_only_both"}


def merged_maps(name):
    """(goodness, the merge's inputs, the reference's two maps as recorded --
    zero counts included --, meta of the sequence)."""
    g, datas = P.auc_merge_sequences()[name]
    meta, fx = P.load_fixture("auc_merge")
    info = meta["sequences"][name]
    assert info["input_sha256"] == P.auc_sequence_digest(g, datas) and info["goodness"] == g
    assert meta["thresholds"] == list(P.AUC_THRESHOLDS)
    maps = tuple(fx["%s.%s" % (name, part)] for part in AUC_PARTS)  # all small enough to be held
    assert same_aucdata(fx, meta["sha256"], name, maps)
    return g, datas, maps, info


@pytest.mark.parametrize("name", MERGE_NAMES)
def test_auc_merge_recorded(name):
    from parameter_server_amd.auc import accuracy_data, evaluate_data
    g, datas, maps, info = merged_maps(name)
    kept = P.auc_without_zeros(maps)
    assert info["zero_count_entries"] == sum(m.size for m in maps[::2]) - sum(k.size for k in kept[::2])
    assert (info["zero_count_entries"] > 0) == name.startswith("zero_")
    # merge: the restatements drop zero counts as the product does, and are
    # the reference's maps in everything else
    for merge in (A.scalar_merge, A.vector_merge):
        assert A.same_data(merge(datas), kept), merge.__name__
    # accuracy and evaluate() as written: on the reference's own maps (the
    # zero counts in) the restatements and the library's host functions are
    # the reference's bits ...
    for th, want in zip(P.AUC_THRESHOLDS, info["accuracy_bits"]):
        for data in (maps, kept):  # ... and a zero count adds 0 to both sums
            assert recorded_double(want) == fb(A.scalar_accuracy(data, g, th)) \
                == fb(A.vector_accuracy(data, g, th)) == fb(accuracy_data(g, *data, threshold=th))
    want = recorded_double(info["evaluate_bits"])
    assert want == fb(A.scalar_evaluate(maps, True)) == fb(A.vector_evaluate(maps, True)) \
        == fb(evaluate_data(*maps, as_written=True))
    # PSG_AUC_BY_KEY has no reference: it stays on the two restatements
    # (tests/test_auc.py)
    dropped = [fb(f(kept, True)) for f in (A.scalar_evaluate, A.vector_evaluate)] \
        + [fb(evaluate_data(*kept, as_written=True))]
    if name in ZERO_ONLY:  # both sides of the boundary
        assert want == "nan" and dropped == [fb(0.5)] * 3
        assert kept[0].size == 0 or kept[2].size == 0
    else:
        assert dropped == [want] * 3
        assert want != "nan"


def test_auc_merge_sequences_cover_what_they_claim():
    seq = P.auc_merge_sequences()
    assert len(seq["three_workers"][1]) == 3
    tk = np.concatenate([d[0] for d in seq["repeated_keys"][1]])
    assert np.unique(tk).size < tk.size and np.any(np.diff(tk) < 0)
    assert any((d[1] == 0).any() and (d[3] == 0).any() for d in seq["zero_counts"][1])
    assert all(d[2].size == 0 for d in seq["no_negatives"][1])
    assert all(d[0].size == 0 for d in seq["no_positives"][1])
    # the double sums are order-sensitive: the counts add up past 2^53
    assert sum(int(d[1].sum()) for d in seq["three_workers"][1]) > 1 << 53
    # (double)key rounds onto x = threshold * goodness on both sides of it
    g, (d,) = seq["keys_past_2p53"]
    x = 0.5 * g
    assert float(int(x) - 1) == x == float(int(x) + 1) and int(x) - 1 in d[0].tolist()


@pytest.mark.parametrize("name", [c.name for c in P.exact_auc_cases()])
def test_exact_auc_recorded(name):
    cases = P.exact_auc_cases()
    meta, fx = P.load_fixture("exact_auc")
    i = [c.name for c in cases].index(name)
    c = cases[i]
    assert meta["cases"][name]["input_sha256"] == c.digest() and list(meta["cases"]) == sorted(
        x.name for x in cases)
    want = recorded_double("%016x" % int(fx["bits"][i]))
    assert (want == "nan") == (c.y.size == 1)  # one class absent: 0 / 0
    assert want == fb(A.scalar_exact(c.y, c.p)) == fb(A.vector_exact(c.y, c.p))
    # the result must not depend on how equal predictions are ordered: every
    # run of equal predictions (-0.0 == +0.0) is of one class
    o = np.argsort(c.p, kind="stable")
    p, pos = c.p[o], c.y[o] > 0
    tie = p[1:] == p[:-1]
    assert np.array_equal(pos[1:][tie], pos[:-1][tie])
    assert tie.any() == name.startswith("ties") or c.y.size == 1
    assert (c.p < 0).any() or c.y.size == 1


# ----------------------------------------------------------------- localizer
LOC_OUT = ("new_offset", "new_index", "new_value", "remapped_idx")
_loc_cache = {}


def loc(name):
    if name not in _loc_cache:
        _loc_cache[name] = P.loc_case(name)
    return _loc_cache[name]


def restated_localizer(c, form):
    """{key: array} as tools/record_reference.py names the outputs."""
    count, remap = {"scalar": (W.scalar_count_uniq, W.scalar_remap),
                    "vector": (W.vector_count_uniq, W.vector_remap)}[form]
    skey, spos, uniq, cnt = count(c.index)
    out = {"uniq_idx": uniq, "idx_frq": cnt}
    for dname, dic in c.dicts.items():
        no, ni, nv, rm = remap(c.offset, c.index, c.value, dic, skey, spos)
        for k, a in zip(LOC_OUT, (no, ni, P.fbits(np.asarray(nv, np.float64)), rm)):
            out["%s.%s" % (dname, k)] = a
    return out


@pytest.mark.parametrize("form", ("scalar", "vector"))
@pytest.mark.parametrize("name", P.LOC_NAMES)
def test_localizer_recorded(name, form):
    c = loc(name)
    meta, fx = P.load_fixture("localizer")
    info = meta["cases"][name]
    assert meta["tile"] == P.PIN_TILE and info["input_sha256"] == c.digest()
    assert (info["nnz"], info["rows"], info["binary"]) == (c.index.size, c.offset.size - 1,
                                                           c.value is None)
    got = restated_localizer(c, form)
    assert got["uniq_idx"].size == info["n_uniq"]
    for k in ("uniq_idx", "idx_frq"):
        assert P.same_output(fx, meta["sha256"], "%s.%s" % (name, k), got[k]), k
    assert sorted(info["matched"]) == sorted(c.dicts)
    for dname, matched in info["matched"].items():
        if dname == "empty":
            # the reference returns a null pointer (localizer.h:114); an empty
            # Z is the product's own defined deviation (include/psg.h)
            assert matched is None and got["empty.new_index"].size == 0
            assert not any(k.startswith("%s.empty." % name) for k in meta["sha256"])
            continue
        assert matched == got[dname + ".new_index"].size
        for k in LOC_OUT:
            assert P.same_output(fx, meta["sha256"], "%s.%s.%s" % (name, dname, k),
                                 got["%s.%s" % (dname, k)]), (dname, k)


def test_localizer_cases_cover_what_they_claim():
    meta, _ = P.load_fixture("localizer")
    T = P.PIN_TILE
    assert [loc(n).index.size for n in P.LOC_NAMES] == [1, T - 1, T, T + 1, 3 * T + 5, 40000, 40000]
    assert meta["threads"] == [1, 4] and 40000 > 4 * (16 * 1024) // 2  # past parallelSort's grain
    assert 40000 // 4 + 5 < 16 * 1024 < 40000  # the grain is 16,384: 40,000 pairs split at least once
    for name in P.LOC_NAMES:
        c = loc(name)
        uniq, cnt = np.unique(c.index, return_counts=True)
        lens = np.diff(c.offset.astype(np.int64))
        if lens.size >= 3:
            assert lens[0] == lens[lens.size // 2] == lens[-1] == 0
        assert (uniq > np.uint64(1 << 63)).any() or name == "L1"
        if name in ("Tm1", "Tp1", "3Tp5", "L40000"):
            assert cnt.max() > 64
        if name in ("T", "D40000"):
            assert cnt.max() == 1
        m = meta["cases"][name]["matched"]
        assert m["all"] == m["absent"] == c.index.size and (0 < m["third"] < c.index.size or name == "L1")
        if "below" in m:
            assert m["below"] == m["above"] == 0
            assert c.dicts["below"].max() < uniq[0] and c.dicts["above"].min() > uniq[-1]
            assert c.dicts["absent"][0] < uniq[0] and c.dicts["absent"][-1] > uniq[-1]
        assert c.dicts["absent"].size > uniq.size or name == "L1"
    assert {0, P.U64 - 1} <= set(loc("3Tp5").index.tolist())
    assert loc("Tp1").offset.size == 2 and loc("L1").offset.size == 2  # single-row cases
    assert {n for n in P.LOC_NAMES if loc(n).value is None} == {"T", "Tp1", "D40000"}
    # too large for the cap: held as a digest only
    _, fx = P.load_fixture("localizer")
    assert "L40000.all.new_index" not in fx and "L40000.all.new_index" in meta["sha256"]


# ---------------------------------------------------------------------- live
@pytest.mark.parametrize("seed", range(8))
def test_live_auc(seed):
    need("auc")
    c = P.random_auc_case(seed)
    want = R.auc_compute(c.y, c.p, c.g)
    assert A.same_data(want, A.scalar_compute(c.y, c.p, c.g))
    assert A.same_data(want, A.vector_compute(c.y, c.p, c.g))
    # a root over the case in three workers' pieces and one list with zero counts
    n = c.y.size
    cuts = [0, n // 3, n // 2, n]
    datas = [R.auc_compute(c.y[a:b], c.p[a:b], c.g) for a, b in zip(cuts, cuts[1:]) if b > a]
    datas.append((want[0][::-1], np.zeros(want[0].size, np.uint64), want[2], want[3]))
    root = R.RefAUC(c.g)
    for d in datas:
        root.merge(*d)
    maps = root.maps()
    kept = P.auc_without_zeros(maps)
    assert A.same_data(kept, A.scalar_merge(datas)) and A.same_data(kept, A.vector_merge(datas))
    from parameter_server_amd.auc import accuracy_data, evaluate_data
    for th in P.AUC_THRESHOLDS + (1.0, -20.0):
        assert fb(root.accuracy(th)) == fb(A.scalar_accuracy(maps, c.g, th)) \
            == fb(A.vector_accuracy(kept, c.g, th)) == fb(accuracy_data(c.g, *kept, threshold=th))
    assert fb(root.evaluate()) == fb(A.scalar_evaluate(maps, True)) \
        == fb(A.vector_evaluate(maps, True)) == fb(evaluate_data(*maps, as_written=True))
    # Evaluation<double>::auc on a tie-free input of the same size
    p = (np.argsort(P.splitmix64(seed, n), kind="stable") - n // 2) * 0.25
    assert fb(R.exact_auc(c.y, p)) == fb(A.scalar_exact(c.y, p)) == fb(A.vector_exact(c.y, p))


@pytest.mark.parametrize("threads", (1, 2, 4))
@pytest.mark.parametrize("seed", range(8))
def test_live_localizer(seed, threads):
    need("localizer")
    c = P.random_loc_case(seed)
    ref = R.RefLocalizer()
    uniq, frq = ref.count_uniq(c.index, threads)
    tag = np.arange(c.index.size, dtype=np.float64)
    for form in ("scalar", "vector") if c.index.size <= 20000 else ("vector",):
        got = restated_localizer(c, form)
        assert same(got["uniq_idx"], uniq) and same(got["idx_frq"], frq)
        for dname, dic in c.dicts.items():
            res = ref.remap(c.offset, c.index, c.value, dic, threads)
            if dname == "empty":
                assert res is None
                continue
            no, ni, nv = res
            assert same(got[dname + ".new_offset"], no) and same(got[dname + ".new_index"], ni)
            assert same(got[dname + ".new_value"], P.fbits(nv))
            tagged = ref.remap(c.offset, c.index, tag, dic, threads)
            assert same(got[dname + ".remapped_idx"],
                        P.remapped_from_tagged(c.index.size, tagged[1], tagged[2]))


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
    # the AUC and localizer fixtures: recorded again, nothing written
    need("auc")
    need("localizer")
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "record_reference", os.path.join(R.ROOT, "tools", "record_reference.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    again = {}
    keep, rec.P.save_fixture = rec.P.save_fixture, lambda name, meta, arrays: again.update(
        {name: (meta, arrays)})
    try:
        rec.record_auc()
        rec.record_localizer()
    finally:
        rec.P.save_fixture = keep
    assert sorted(again) == ["auc", "auc_merge", "exact_auc", "localizer"]
    for name, (meta, arrays) in again.items():
        wmeta, warrays = P.load_fixture(name)
        assert json_round(meta) == wmeta and sorted(arrays) == sorted(warrays), name
        assert all(same(arrays[k], warrays[k]) and arrays[k].dtype == warrays[k].dtype
                   for k in arrays), name


def json_round(meta):
    import json
    return json.loads(json.dumps(meta, sort_keys=True))


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
