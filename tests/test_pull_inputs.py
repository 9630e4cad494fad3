"""The pull-path seam inputs (tests/pull_inputs.py) reach the seams their
names claim, and the oracles agree on them (no GPU).

test_pull_edges_gpu.py trusts the builders to put a repeat on a lane seam, a
span at 4,096 keys, an inversion at index 1,024 and so on.  These tests
restate each claim with np.searchsorted and index arithmetic, so that a
change to a builder cannot quietly empty a GPU test.  They also hold the
expected values to two more statements of the rule: a few lines of NumPy
(pull_inputs.numpy_gather, np.searchsorted for the slice) and, where
oracle/_ref holds it, the reference's own code compiled in place."""
import numpy as np
import pytest

import oracle_py as O
import pull_inputs as P
import ref_py as R

DTYPES = (np.float32, np.float64)
GATHER_FAMILIES = (P.family_a, P.family_b, P.family_c, P.family_d, P.family_f)


def gather_cases(dtype):
    out = [c for fam in GATHER_FAMILIES for c in fam(dtype)]
    out += [c[:4] for c in P.family_e(dtype) if c[5] == "equal"]
    return out


def is_sorted(a):
    return bool(np.all(a[1:] >= a[:-1]))


def test_constants_match_the_kernels():
    """The mirrored constants are the ones psg_kernels.hip defines."""
    import os
    import re
    src = open(os.path.join(O.ROOT, "parameter_server_amd", "csrc", "psg_kernels.hip")).read()
    assert int(re.search(r"constexpr int kGR = (\d+);", src).group(1)) == P.GR
    assert int(re.search(r"constexpr int kGS = (\d+);", src).group(1)) == P.GS
    assert "constexpr int kI = kGR / 256;" in src
    assert P.PER_THREAD == P.GR // 256 and P.WAVE == 64 * P.PER_THREAD
    assert P.D_SIZES == [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 262143, 262144, 262145]


def test_inputs_are_well_formed():
    names = set()
    for dtype in DTYPES:
        for name, D, W, req in gather_cases(dtype):
            names.add(name)
            assert D.dtype == req.dtype == np.uint64 and W.dtype == dtype, name
            assert W.size == D.size and np.all(D[1:] > D[:-1]), name
            assert 1 <= req.size <= 5000 and D.size <= 262145 and is_sorted(req), name
    assert len(names) == len(gather_cases(np.float32))  # names are unique


def test_special_values_are_requested():
    """-0.0, +inf, -inf and the payload NaN sit where requests read them."""
    for dtype in DTYPES:
        sp = P.special_bits(dtype).tolist()
        for name, D, W, req in gather_cases(dtype):
            want, matched = O.gather(D, W, req, dtype)
            read = set(P.bits(want).tolist())
            assert set(sp[:min(matched, 4)]) <= read, name


def test_family_a_counts():
    cases = P.family_a(np.float32)
    assert [c[3].size for c in cases] == [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025,
                                          2047, 2048, 2049, 3073]
    for name, D, W, req in cases:
        assert D.size == 20000 and np.unique(req).size == req.size, name
        present = int(np.isin(req, D).sum())
        assert 0 < present and abs(3 * present - 2 * req.size) <= 3, name
        assert present < req.size or req.size == 1, name


def test_family_b_repeats_sit_on_their_seams():
    D, req = P.repeat_request()
    assert req.size == 2100 and D.size == 20000 and is_sorted(req)
    rep = P.REPEATS_B
    for i in rep["thread"]:
        assert i % P.PER_THREAD in (1, 2, 3)
    for i in rep["lane"]:
        assert i % P.PER_THREAD == 0 and i % P.WAVE != 0
    for i in rep["wave"] + rep["absent_wave"]:
        assert i % P.WAVE == 0 and i % P.GR != 0
    assert rep["workgroup"] == [P.GR, 2 * P.GR]
    assert rep["triple"] == [P.GR, P.GR + 1]
    assert {i % P.PER_THREAD for i in rep["thread"]} == {1, 2, 3}
    # the repeats are exactly the listed ones
    listed = sorted({i for v in rep.values() for i in v})
    assert (np.flatnonzero(req[1:] == req[:-1]) + 1).tolist() == listed
    assert req[1023] == req[1024] == req[1025]
    present = np.isin(req, D)
    for kind, at in rep.items():
        for i in at:
            assert present[i] == (kind != "absent_wave"), (kind, i)
    assert 0 < int((~present).sum()) < req.size
    # second case: one key fills a workgroup and runs on into the next
    name, D2, W2, req2 = P.family_b(np.float32)[1]
    assert req2.size == P.B2_COPIES + P.B2_TAIL and P.B2_COPIES > P.GR
    assert np.all(req2[:P.B2_COPIES] == req2[0]) and np.all(np.isin(req2, D2))
    tail = req2[P.B2_COPIES - 1:]
    assert np.all(tail[1:] > tail[:-1])
    assert P.spans(D2, req2)[0] == 1


def test_family_c_spans_are_exact():
    cases = P.family_c(np.float32)
    assert {c[0] for c in cases} == set(P.C_SPANS)
    for name, D, W, req in cases:
        assert np.all(np.diff(D.astype(np.int64)) == P.C_STEP) and P.C_STEP > P.GR + 1
        assert np.unique(req).size == req.size, name
        got, want = P.spans(D, req), P.C_SPANS[name]
        assert len(got) == len(want) and req.size == P.GR * len(want), name
        for g, w in zip(got, want):
            assert (g > 2 * P.GS) if w is None else (g == w), (name, got)
        if name.startswith("c_span") and want[0] >= 1:
            lo = int(np.searchsorted(D, req[0]))
            first, last = D[lo], D[lo + want[0] - 1]
            assert first in req and last in req, name
            if name.endswith("absent_top"):
                assert req[-1] == last + np.uint64(1) and req[-1] not in D, name
                assert want[0] == 1 or req[-2] == last, name
            else:
                assert req[-1] == last, name
    by = {c[0]: c for c in cases}
    D = by["c_span0_gap"][1]
    r = by["c_span0_gap"][3]
    lo = int(np.searchsorted(D, r[0]))
    assert 0 < lo < D.size and D[lo - 1] < r[0] and r[-1] < D[lo]
    assert by["c_span0_below"][3][-1] < D[0] and by["c_span0_above"][3][0] > D[-1]
    assert sorted({P.C_SPANS[c[0]][0] for c in cases if len(P.C_SPANS[c[0]]) == 1}) == \
        [0, 1, 4095, 4096, 4097]


def test_family_d_requests():
    cases = {c[0]: c for c in P.family_d(np.float32)}
    assert [cases["d_nd%d" % n][1].size for n in P.D_SIZES] == P.D_SIZES
    for name, D, W, req in cases.values():
        assert np.unique(req).size == req.size and req[0] == 0 and req[-1] == P.U64_MAX, name
        have = set(req.tolist())
        n = D.size
        want = []
        if n:
            want += [int(D[0]), int(D[min(1, n - 1)]), int(D[-1])]
            if D[0] > 0:
                want.append(int(D[0]) - 1)
            if D[-1] < P.U64_MAX:
                want.append(int(D[-1]) + 1)
        for p in (62, 63, 64, 65, 4094, 4095, 4096, 4097, n // 2):
            if p < n:
                want += [int(D[p]) + d for d in (-1, 0, 1) if 0 <= int(D[p]) + d <= P.U64_MAX]
        assert set(want) | {0, P.U64_MAX} == have, name
    assert cases["d_key_zero"][1][0] == 0 and cases["d_key_max"][1][-1] == P.U64_MAX
    # both are requested, and read a value
    assert O.gather(*cases["d_key_zero"][1:4])[1] == O.gather(*cases["d_key_max"][1:4])[1] > 0
    assert P.bits(cases["d_key_zero"][2])[0] != 0 and P.bits(cases["d_key_max"][2])[-1] != 0


def test_family_e_one_inversion_or_none():
    cases = P.family_e(np.float32)
    assert [c[4] for c in cases if c[5] == "swap"] == P.ORDER_AT == \
        [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2099]
    assert [c[4] for c in cases if c[5] == "equal"] == P.ORDER_AT
    for name, D, W, req, i, kind in cases:
        assert req.size == 2100 and np.all(np.isin(req, D)), name
        down = np.flatnonzero(req[1:] < req[:-1]) + 1
        same = np.flatnonzero(req[1:] == req[:-1]) + 1
        if kind == "swap":
            assert down.tolist() == [i] and same.size == 0, name
            assert np.unique(req).size == req.size, name
        else:
            assert down.size == 0 and same.tolist() == [i], name
    at = set(P.ORDER_AT)
    assert {P.SORT_BLOCK, P.GR} <= at            # workgroup seams of both order checks
    assert {64, 1, P.SORT_BLOCK - 1, P.SORT_BLOCK + 1, P.GR - 1, P.GR + 1} <= at


def test_family_f_matched_counts():
    cases = P.family_f(np.float64)
    assert [c[3].size for c in cases] == [700, 2500, 1024, 4100, 1025]
    assert [(c[3].size + P.GR - 1) // P.GR for c in cases] == [1, 3, 1, 5, 2]
    counts = [O.gather(D, W, req, np.float64)[1] for _, D, W, req in cases]
    assert len(set(counts)) == len(counts)
    for m, c in zip(counts, cases):
        assert 0 < m < c[3].size
        assert c[1] is cases[0][1] and c[2] is cases[0][2]  # one D, one W


def test_family_g_separators():
    cases = P.family_g()
    assert len(cases) == len(P.D_SIZES) * len(P.NSEP_G) * 2
    assert sorted({c[4].size for c in cases}) == [1, 2, 3, 4, 5, 9]
    assert max(P.NSEP_G) > 2 * P.SLICE_WAVES  # three workgroups, the last one partial
    kinds = set()
    for name, D, kb, ke, sep in cases:
        assert kb < ke and is_sorted(sep), name
        if "inner" in name:
            assert kb not in D and ke not in D and kb > 0 and ke < P.U64_MAX, name
        for s in sep.tolist():
            kinds.add("zero" if s == 0 else "max" if s == P.U64_MAX else "below" if s < kb
                      else "above" if s > ke else "kb" if s == kb else "ke" if s == ke
                      else "key" if s in D else "key+1" if s - 1 in D else "other")
    assert kinds >= {"zero", "max", "below", "above", "kb", "ke", "key", "key+1"}


# ------------------------------------------------------- oracle agreement --
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_oracle_matches_numpy_rule(dtype):
    for name, D, W, req in gather_cases(dtype):
        want, wm = O.gather(D, W, req, dtype)
        got, gm = P.numpy_gather(D, W, req)
        assert gm == wm, name
        assert np.array_equal(P.bits(got), P.bits(want)), name
        # an absent or repeated request reads +0.0: the sign bit is clear
        rep = np.zeros(req.size, bool)
        rep[1:] = req[1:] == req[:-1]
        assert not P.bits(want)[rep | ~np.isin(req, D)].any(), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_oracle_matches_reference(dtype):
    if not R.available("match"):
        pytest.skip("oracle/_ref/%s not built (reference tree absent)" % R.LIBS["match"])
    top = np.uint64(P.U64_MAX)
    checked = 0
    for name, D, W, req in gather_cases(dtype):
        # the reference's key ranges are half-open in uint64, so none of them
        # holds the key 2^64 - 1: it is taken out of both sides here
        D, W, req = D[D < top], W[D < top], req[req < top]
        want, wm = O.gather(D, W, req, dtype)
        got, gm = R.gather(D, W, req, dtype)
        assert gm == wm, name
        assert np.array_equal(P.bits(got), P.bits(want)), name
        checked += wm
    assert checked > 10000


def test_slice_oracle_matches_searchsorted():
    for name, D, kb, ke, sep in P.family_g():
        pos, _ = O.slice_key_ordered(D, kb, ke, sep)
        k = np.clip(sep, np.uint64(kb), np.uint64(ke))
        assert np.array_equal(pos, np.searchsorted(D, k, "left").astype(np.uint64)), name


def test_slice_oracle_matches_reference():
    if not R.available("match"):
        pytest.skip("oracle/_ref/%s not built (reference tree absent)" % R.LIBS["match"])
    checked = 0
    for name, D, kb, ke, sep in P.family_g():
        if sep.size < 2:
            continue  # sliceKeyOrderedMsg cuts between separators: it needs two
        pos, ovalid = O.slice_key_ordered(D, kb, ke, sep)
        b, e, vb, valid = R.slice_key_ordered(D, kb, ke, sep)
        assert np.array_equal(ovalid, valid), name
        ok = valid == 1
        assert np.array_equal(pos[:-1][ok].astype(np.int64), b[ok]), name
        assert np.array_equal(pos[1:][ok].astype(np.int64), e[ok]), name
        checked += int(ok.sum())
    assert checked > 100
