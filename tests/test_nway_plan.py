"""CPU: the N-way merge's planner (psg_nway_plan.h through psg_nway_shape)
against the plain-integer model of tests/nway_ref.py, and the model's own
properties: for sorted pushes the tile sizes sum to sum(n) and none passes a
tile's 2,048 elements (psg_nway.hip's header); for disordered pushes -- the
cases of tests/test_nway_edges_gpu.py -- some tile overflows, which is what
the device must report as PSG_ERR_UNSORTED and not as a device fault."""
import numpy as np
import pytest

import nway_ref as R
from pin_cases import splitmix64


def _lib_plan(merges_ns):
    from parameter_server_amd.kv_vector import nway_shape
    return nway_shape(merges_ns)


def _model_plan(merges_ns):
    sh, form, rr, _ = R.batch_plan(merges_ns)
    return [(x["K"], x["s"], x["cw"], x["B"], x["T"]) for x in sh], form, rr


def _ragged(seed, K):
    """K push lengths around the merge's stride seams, with empty pushes."""
    s = max(1, R.CAP // (8 * K))
    seam = [0, 1, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, 5 * s + 3, 40 * s]
    r = splitmix64(seed, K)
    return [seam[int(x % np.uint64(len(seam)))] for x in r]


def test_shape_matches_library_over_push_counts():
    """K = 1..64 non-empty pushes (more with the empty ones) of ragged
    lengths, one merge each and all of them as one batch."""
    merges = []
    for K in range(1, 65):
        for rep in range(3):
            ns = _ragged(1000 * K + rep, K)
            if rep == 2:
                ns = [0] + ns + [0, 0]  # empty pushes are dropped, not counted
            if rep == 1:
                ns = [n or 1 for n in ns]  # exactly K kept
            merges.append(ns)
            assert _lib_plan([ns]) == _model_plan([ns]), ns
    got = _lib_plan(merges)
    assert got == _model_plan(merges)
    kept = [k for (k, _, _, _, _) in got[0]]
    assert max(kept) == 64 and min(kept) >= 0
    # a merge of no (non-empty) pushes has no buckets and no tiles
    assert _lib_plan([[0, 0], [5]])[0][0] == (0, 2048 // 8, 2048, 0, 0)


def test_shape_argument_errors():
    from parameter_server_amd._lib import PSG_ERR_ARG, PSGError
    with pytest.raises(PSGError) as e:
        _lib_plan([[1] * 65])
    assert e.value.status == PSG_ERR_ARG
    with pytest.raises(PSGError) as e:
        _lib_plan([[1 << 31, 1 << 31]])
    assert e.value.status == PSG_ERR_ARG
    assert _lib_plan([[0] * 70 + [1] * 64])[0][0][0] == 64


@pytest.mark.parametrize("merges,form", [
    (R.form16_lengths(), 16),
    ([[200] * 64] * 128, 4),
    ([[131072] * 8], 1),
    ([[300, 300]] * 511 + [[8192 * 128, 8193 * 128]], 16),
])
def test_rank_form_of_batches(merges, form):
    """The batches of tests/test_nway_edges_gpu.py's rank-form cases."""
    shapes, got, rr = _lib_plan(merges)
    assert (shapes, got, rr) == _model_plan(merges)
    assert got == form


def _sorted_merges():
    yield [np.arange(600, dtype=np.uint64)] * 3            # the fullest tile found: 1,782
    yield [np.arange(48, dtype=np.uint64) * np.uint64(5)] * 64
    for K in (1, 2, 3, 8, 33, 64):
        ns = [n for n in _ragged(77 + K, K) if n] or [1]
        yield [R.sorted_keys(900 + 64 * K + q, n, 24) for q, n in enumerate(ns)]
        yield [R.sorted_keys(7 + q, 300 + 13 * q, 64) for q in range(K)]
    # clustered keys: most in a narrow range
    c = np.unique(np.concatenate([np.arange(1 << 40, (1 << 40) + 9000, dtype=np.uint64),
                                  splitmix64(5, 50) >> np.uint64(1)]))
    yield [c[q::3] for q in range(3)] + [c]


def test_sorted_pushes_fill_no_tile_and_lose_nothing():
    fullest = 0
    for pushes in _sorted_merges():
        m = R.Merge(pushes)
        assert sum(m.tile_sizes) == m.ntot
        assert max(m.tile_sizes) <= R.CAP
        assert all(a <= b for a, b in zip(m.split, m.split[1:]))
        fullest = max(fullest, max(m.tile_sizes))
        # the kernels' search, transcribed, is a lower bound on sorted arrays
        d = R.Merge(pushes, device=True)
        assert (d.split, d.seg, d.rank) == (m.split, m.seg, m.rank)
    assert fullest == 1782


def test_interp_lower_bound_transcription():
    """Exact on sorted arrays of every length around the 16-key tail and on
    the extreme keys; inside [0, n] on disordered ones."""
    for n in (1, 2, 15, 16, 17, 18, 33, 100, 1000):
        k = R.sorted_keys(n, n, 20)
        probes = np.unique(np.concatenate([k, k + np.uint64(1), k[:1] - np.uint64(1) * (k[:1] > 0)]))
        want = np.searchsorted(k, probes, "left").tolist()
        assert [R.interp_lower_bound(k.tolist(), int(x)) for x in probes] == want
    edge = [0, 1, 1 << 63, R.M64 - 1, R.M64]
    assert [R.interp_lower_bound(edge, x) for x in edge] == [0, 1, 2, 3, 4]
    wide = [0] + list(range(1 << 40, (1 << 40) + 40)) + [R.M64]
    assert R.interp_lower_bound(wide, (1 << 40) + 17) == 18
    for pushes in (R.case_b(), R.case_reversed(), R.case_c(3)):
        S = pushes[1].tolist()
        for x in pushes[0][::97].tolist():
            assert 0 <= R.interp_lower_bound(S, x) <= len(S)
    assert R._f2u64(float("nan")) == 0 and R._f2u64(-1.0) == 0 and R._f2u64(2.0 ** 70) == R.M64


@pytest.mark.parametrize("case,tile,size", [("case_a", 3, 6254), ("case_b", 1, 6234),
                                            ("case_reversed", 6, 6000)])
def test_disordered_cases_overflow_a_tile(case, tile, size):
    m = R.Merge(getattr(R, case)(), device=True)
    assert m.shape["T"] == 7
    assert m.overflows() == [tile] and m.tile_sizes[tile] == size
    # what the tiles that are merged hold fits sum(n): these cases may go
    # through the unions whose output the library sizes
    assert m.kept_elements() <= m.ntot


def test_duplicate_run_overflows_nothing():
    """400 equal keys: disordered, yet every tile fits -- the tile kernel's
    own order check reports it."""
    m = R.Merge(R.case_dup_run(), device=True)
    assert m.overflows() == [] and sum(m.tile_sizes) == m.ntot


def test_block_move_search_finds_an_overflow():
    seed, pushes = R.search_case_c(lambda m: bool(m.overflows()))
    assert seed == R.CASE_C_OVERFLOW_SEED
    assert np.array_equal(np.sort(pushes[1]), np.unique(pushes[1]))  # a permutation of a sorted push
    hits = sum(bool(R.Merge(R.case_c(s), device=True).overflows()) for s in range(80))
    assert hits >= 3


def test_block_move_search_finds_an_over_producing_input():
    """The tiles that do not overflow hold more different keys than sum(n)
    (pieces of the disordered push overlap): more than out_keys holds, which
    is why the tile kernel bounds its compacted write.  The search from seed
    0 first hits at CASE_C_OVERPRODUCE_SEED; here its last stretch."""
    last = R.CASE_C_OVERPRODUCE_SEED
    seed, pushes = R.search_case_c(lambda m: m.distinct() > m.ntot, range(last - 40, last + 1))
    assert seed == last
    m = R.Merge(pushes, device=True)
    assert m.overflows() == []
    assert m.distinct() - m.ntot == 258 and sum(m.tile_sizes) - m.ntot == 408
