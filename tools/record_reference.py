#!/usr/bin/env python3
"""Record the reference's own outputs into tests/golden/reference_pin/.

Runs the reference's code compiled in place (oracle/_ref/libref_match.so,
libref_ftrl.so, libref_countmin.so, libref_auc.so, libref_localizer.so --
`make -C oracle` with the reference tree present) on the fixed inputs of tests/pin_cases.py and stores what it
returns as data-only fixtures (numpy .npz: little-endian arrays and a JSON
`meta` holding parameters, digests and the source).  Run by hand when the
cases change; no test calls it.  A fixture is never edited to fit: if a
restatement or a kernel disagrees with one, the code is what changes.

    python tools/record_reference.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pin_cases as P  # noqa: E402
import ref_py as R  # noqa: E402

MAX_BYTES = 128 * 1024
SOURCE = {
    "fold": "reference src/system/message.h:89-267 (match, oldMatch, sliceKeyOrderedMsg) and "
            "src/base/range.h:85-98 compiled in place (oracle/ref_match_shim.cc); the per-push "
            "loops follow src/parameter/kv_vector.h:106-132,185-201,216-227",
    "ftrl": "reference src/linear_method/ftrl_model.h with src/base/soft_thresholding.h compiled "
            "in place (oracle/ref_ftrl_shim.cc)",
    "countmin": "reference src/parameter/frequency_filter.h with src/base/countmin.h compiled in "
                "place (oracle/ref_countmin_shim.cc)",
    "auc": "reference src/base/auc.h (setGoodness, compute, merge, accuracy, evaluate) and "
           "src/base/evaluation.h (Evaluation<double>::auc) compiled in place "
           "(oracle/ref_auc_shim.cc)",
    "localizer": "reference src/base/localizer.h (countUniqIndex, remapIndex) over "
                 "src/util/parallel_sort.h compiled in place (oracle/ref_localizer_shim.cc)",
}


def same_bits(a, b):
    return all(np.array_equal(P.fbits(x), P.fbits(y)) for x, y in zip(a, b))


def record_even_divide():
    b, e = R.range_all()
    assert (b, e) == (0, P.U64)
    arrays = {}
    for n in P.EVEN_DIVIDE_N:
        bounds = np.array([R.even_divide(b, e, n, i) for i in range(n)], np.uint64)
        arrays["n%d" % n] = bounds  # [n, 2]: (begin, end) of piece i
    P.save_fixture("even_divide", {"source": SOURCE["fold"], "range_all": [b, e],
                                   "n": list(P.EVEN_DIVIDE_N)}, arrays)
    return arrays["n8"]


def record_fold(bounds8):
    sep = np.concatenate([bounds8[:, 0], bounds8[-1:, 1]])
    for name in P.FOLD_NAMES:
        c = P.fold_case(name)
        for r, (kb, ke) in enumerate(c.ranges):
            pushes = c.sliced(r)
            arrays, meta = {}, {"source": SOURCE["fold"], "case": name, "dtype": c.dtype.name,
                                "m": c.m, "key_range": [kb, ke], "npush": len(pushes),
                                "input_sha256": c.digest(), "parallel_threads": 2}
            rc, lo, hi, ser, mt = R.aggregate(c.D, kb, ke, pushes, False, 1, c.dtype)
            assert rc == 0 and mt.tolist() == [k.size for k, _ in pushes]
            rc, plo, phi, par, pmt = R.aggregate(c.D, kb, ke, pushes, True, 2, c.dtype)
            assert rc == 0 and (plo, phi) == (lo, hi) and pmt.tolist() == mt.tolist()
            for t in (1, 4):  # the thread count must not show in the bytes
                rc, _, _, other, omt = R.aggregate(c.D, kb, ke, pushes, True, t, c.dtype)
                assert rc == 0 and same_bits(other, par) and omt.tolist() == mt.tolist()
            meta["positions"] = [lo, hi]
            arrays["matched"] = mt
            for i in range(c.m):
                arrays["serial%d" % i] = P.fbits(ser[i])
                arrays["parallel%d" % i] = P.fbits(par[i])
            meta["serial_differs_from_parallel"] = int(sum(
                np.count_nonzero(P.fbits(ser[i]) != P.fbits(par[i])) for i in range(c.m)))
            out, gm = R.gather(c.D, c.W, c.R, c.dtype)
            arrays["gather"] = P.fbits(out)
            meta["gather_matched"] = gm
            b, e, vb, valid = R.slice_key_ordered(c.D, kb, ke, sep)
            assert np.array_equal(b, vb)
            arrays["slice_begin"], arrays["slice_end"], arrays["slice_valid"] = b, e, valid
            arrays["slice_sep"] = sep
            P.save_fixture(c.fixture(r), meta, arrays)


def run_ftrl(model, msgs, keys):
    after = []
    for msg in msgs:
        model.push(*msg)
        after.append({"size": model.entries, "nnz": model.nnz,
                      "entries_sha256": P.entry_digest(*model.lookup(keys))})
    return after


def record_ftrl():
    c = P.ftrl_case()
    for k, pos, neg, g in c.msgs[:1]:
        assert np.isin(c.last_bucket, k).all() and np.isin(c.bucket0, k).all()
    assert sum(int((m[1] == 0xFFFFFFFF).sum()) for m in c.msgs) >= 6
    allg = np.concatenate([m[3] for m in c.msgs])
    assert np.isnan(allg).any() and (allg == np.inf).any() and (allg == -np.inf).any()
    assert (allg == 5e-324).any() and (P.fbits(allg) == np.uint64(1 << 63)).any()
    for pname, param in P.FTRL_PARAMS.items():
        m = R.RefFTRL(**param)
        meta = {"source": SOURCE["ftrl"], "param": param, "input_sha256": c.digest(),
                "nkeys": int(c.keys.size), "request": int(c.request.size)}
        meta["after"] = run_ftrl(m, c.msgs, c.keys)
        pos, neg, w, z, found = m.lookup(c.keys)
        assert 0 < int(found.sum()) < found.size  # some keys are in no message
        arrays = {"pos": pos, "neg": neg, "w": P.fbits(w), "z": P.fbits(z), "found": found}
        # in this order: the reference's pull inserts
        meta["objv_bits"] = "%016x" % int(P.fbits(np.array([m.objv()]))[0])
        text = P.sorted_dump(m.dump_text())
        arrays["dump_text"] = np.frombuffer(text.encode(), np.uint8)
        arrays["pull"] = P.fbits(m.get_value(c.request))
        meta["size_after_pull"] = m.entries
        # the same without the two infinite-gradient keys: a finite objv
        fm = R.RefFTRL(**param)
        for msg in c.finite_msgs():
            fm.push(*msg)
        meta["finite_objv_bits"] = "%016x" % int(P.fbits(np.array([fm.objv()]))[0])
        meta["finite_nnz"] = fm.nnz
        P.save_fixture("ftrl_" + pname, meta, arrays)


def record_countmin():
    arrays, meta = {}, {"source": SOURCE["countmin"], "shapes": [list(s) for s in P.CM_SHAPES],
                        "freqs": list(P.CM_FREQS), "cases": {}}
    for n, k in P.CM_SHAPES:
        c = P.cm_case(n, k)
        tag = "n%d_k%d" % (n, k)
        f = R.RefFilter()
        info = {"input_sha256": c.digest(), "empty_before_resize": f.empty()}
        f.resize(n, k)
        info["empty_after_resize"] = f.empty()
        for keys, counts in c.batches:
            f.insert_keys(keys, counts)
        info["n_"], info["k_"], table = f.table()
        arrays[tag + "_table"] = table
        info["kept"] = {}
        for freq in P.CM_FREQS:
            kept = f.query_keys(c.query, freq)
            # queryKeys keeps the input order, so a mask over the query says
            # which keys; the kept keys' digest pins the order
            mask = np.zeros(c.query.size, bool)
            j = 0
            for i, q in enumerate(c.query.tolist()):
                if j < kept.size and int(kept[j]) == q:
                    mask[i] = True
                    j += 1
            assert j == kept.size and np.array_equal(c.query[mask], kept)
            arrays["%s_kept%d" % (tag, freq)] = np.packbits(mask)
            info["kept"][str(freq)] = {"n": int(kept.size), "sha256": P.sha256([kept])}
        f.clear()
        info["empty_after_clear"] = f.empty()
        meta["cases"][tag] = info
    P.save_fixture("countmin", meta, arrays)


def hexbits(v):
    return "%016x" % int(P.fbits(np.array([v], np.float64))[0])


def record_auc():
    """auc.npz: compute's AUCData per case; auc_merge.npz: the root's maps,
    accuracy and evaluate per merge sequence; exact_auc.npz: Evaluation::auc."""
    arrays, sha, cases = {}, {}, {}
    for c in P.auc_cases():
        tk, tc, fk, fc = R.auc_compute(c.y, c.p, c.g)
        assert int(tc.sum()) + int(fc.sum()) == c.y.size
        for part, a in (("tp_key", tk), ("tp_count", tc), ("fp_key", fk), ("fp_count", fc)):
            P.record_output(arrays, sha, "%s.%s" % (c.name, part), a)
        cases[c.name] = {"input_sha256": c.digest(), "n": int(c.y.size), "goodness": c.g,
                         "ntp": int(tk.size), "nfp": int(fk.size)}
    # what this build of the reference returns for each undefined conversion
    # on its own (one positive example): the key of its only entry
    for g in P.AUC_GOODNESS:
        keys = [int(R.auc_compute([1.0], [p], g)[0][0]) for p in P.auc_undefined(g)]
        arrays["undefined_g%d.single_keys" % g] = np.array(keys, np.int64)
    P.save_fixture("auc", {"source": SOURCE["auc"], "tile": P.PIN_TILE, "cases": cases,
                           "goodness": list(P.AUC_GOODNESS), "sha256": sha}, arrays)

    arrays, sha, seqs = {}, {}, {}
    for name, (g, datas) in P.auc_merge_sequences().items():
        root = R.RefAUC(g)
        for d in datas:
            root.merge(*d)
        maps = root.maps()
        for part, a in zip(("tp_key", "tp_count", "fp_key", "fp_count"), maps):
            P.record_output(arrays, sha, "%s.%s" % (name, part), a)
        seqs[name] = {"input_sha256": P.auc_sequence_digest(g, datas), "goodness": g,
                      "accuracy_bits": [hexbits(root.accuracy(t)) for t in P.AUC_THRESHOLDS],
                      "evaluate_bits": hexbits(root.evaluate()),
                      "zero_count_entries": int((maps[1] == 0).sum() + (maps[3] == 0).sum())}
    P.save_fixture("auc_merge", {"source": SOURCE["auc"], "thresholds": list(P.AUC_THRESHOLDS),
                                 "sequences": seqs, "sha256": sha}, arrays)

    cases = P.exact_auc_cases()
    bits = np.array([int(hexbits(R.exact_auc(c.y, c.p)), 16) for c in cases], np.uint64)
    P.save_fixture("exact_auc", {"source": SOURCE["auc"], "tile": P.PIN_TILE,
                                 "cases": {c.name: {"input_sha256": c.digest(), "n": int(c.y.size)}
                                           for c in cases}}, {"bits": bits})


def run_localizer(c, threads):
    """{key: array} of everything the reference returns for case c, and
    {dictionary: matched, or None where remapIndex returns a null pointer}."""
    loc = R.RefLocalizer()
    uniq, frq = loc.count_uniq(c.index, threads)
    out, matched = {"uniq_idx": uniq, "idx_frq": frq}, {}
    tag = np.arange(c.index.size, dtype=np.float64)
    for dname in sorted(c.dicts):
        res = loc.remap(c.offset, c.index, c.value, c.dicts[dname], threads)
        tagged = loc.remap(c.offset, c.index, tag, c.dicts[dname], threads)
        if res is None:
            assert tagged is None
            matched[dname] = None
            continue
        no, ni, nv = res
        assert np.array_equal(tagged[0], no) and np.array_equal(tagged[1], ni)
        assert nv.size == (0 if c.value is None else ni.size)
        matched[dname] = int(ni.size)
        out[dname + ".new_offset"], out[dname + ".new_index"] = no, ni
        out[dname + ".new_value"] = P.fbits(nv)
        out[dname + ".remapped_idx"] = P.remapped_from_tagged(c.index.size, tagged[1], tagged[2])
    return out, matched


def record_localizer():
    arrays, sha, cases = {}, {}, {}
    for name in P.LOC_NAMES:
        c = P.loc_case(name)
        out, matched = run_localizer(c, P.LOC_THREADS[0])
        for t in P.LOC_THREADS[1:]:  # the thread count must not show
            other, om = run_localizer(c, t)
            assert om == matched and sorted(other) == sorted(out)
            assert all(np.array_equal(out[k], other[k]) for k in out), (name, t)
        for k, a in out.items():
            P.record_output(arrays, sha, "%s.%s" % (name, k), a)
        cases[name] = {"input_sha256": c.digest(), "nnz": int(c.index.size),
                       "rows": int(c.offset.size - 1), "binary": c.value is None,
                       "n_uniq": int(out["uniq_idx"].size), "matched": matched}
    P.save_fixture("localizer", {"source": SOURCE["localizer"], "tile": P.PIN_TILE,
                                 "threads": list(P.LOC_THREADS), "cases": cases, "sha256": sha},
                   arrays)


def main():
    for which in R.LIBS:
        if not R.available(which):
            sys.exit("%s missing: run `make -C oracle` with the reference tree present"
                     % R.path(which))
    bounds8 = record_even_divide()
    record_fold(bounds8)
    record_ftrl()
    record_countmin()
    record_auc()
    record_localizer()
    for f in sorted(os.listdir(P.GOLDEN)):
        size = os.path.getsize(os.path.join(P.GOLDEN, f))
        print("%-28s %7d bytes" % (f, size))
        assert size <= MAX_BYTES, f


if __name__ == "__main__":
    main()
