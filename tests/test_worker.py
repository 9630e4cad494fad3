"""CPU: the worker step's restatement (tests/worker_ref.py) and its binding.

The restatement is this feature's oracle.  Its localizer part is pinned to
the reference's compiled code in tests/test_reference_pin.py; countKeys,
rangeTimes and LogitLoss are not (worker_ref.py says why), so the whole of it
is also held to itself here: its two independent forms must agree bit for bit on every case the GPU
tests use, its sums must be order-sensitive enough for a bit-exact
comparison to mean something, and its case generators must take every branch
the GPU tests name."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import worker_ref as R
from parameter_server_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096  # test_worker_gpu.py takes it from the library; the forms do not depend on it


def same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        return np.array_equal(R.bits(a), R.bits(b))
    return np.array_equal(a, b)


def both(offset, index, value, y, dic, w):
    a = R.Step("scalar", offset, index, value, y, dic, w)
    b = R.Step("vector", offset, index, value, y, dic, w)
    for k, v in a.arrays().items():
        assert same(v, b.arrays()[k]), k
    assert R.bits(np.float64(a.objv)) == R.bits(np.float64(b.objv))
    return a


def minibatches():
    yield "zipf", R.zipf_case()
    yield "zipf_binary", R.zipf_case(binary=True)
    yield "zipf_odd_labels", R.zipf_case(kinds=R.ODD_LABELS)
    yield "column", R.column_case(rows=400)
    for i, mb in enumerate(R.closed_loop_batches(nbatch=2)):
        yield "loop%d" % i, mb


@pytest.mark.parametrize("name", [n for n, _ in minibatches()])
def test_forms_agree_on_minibatches(name):
    offset, index, value, y = dict(minibatches())[name]
    uniq = np.unique(index)
    for dname, dic in R.dict_cases(uniq).items():
        rng = np.random.default_rng(5)
        w = R.special_vector(rng, dic.size) * 2.0 ** -22
        st = both(offset, index, value, y, dic, w)
        assert np.array_equal(st.uniq, uniq)
        assert int(st.new_offset[-1]) == st.new_index.size


def test_forms_agree_on_sort_cases():
    for name, index in R.sort_cases(TILE).items():
        a, b = R.scalar_count_uniq(index), R.vector_count_uniq(index)
        for x, y in zip(a, b):
            assert same(x, y), name
        skey, spos, uniq, cnt = a
        assert np.all(uniq[1:] > uniq[:-1]) and int(cnt.sum()) == index.size
        # stable: inside a run the positions ascend
        inside = skey[1:] == skey[:-1]
        assert np.all(spos[1:][inside] > spos[:-1][inside]), name


def test_sort_cases_make_every_pass_matter():
    c = R.sort_cases(TILE)
    differ = {k: int(np.bitwise_or.reduce(v) ^ np.bitwise_and.reduce(v)) for k, v in c.items()}
    assert differ["one_key"] == 0                                  # no pass at all
    assert differ["top_byte"] >> 56 and not differ["top_byte"] & ((1 << 56) - 1)
    assert differ["bottom_byte"] & 0xFF and not differ["bottom_byte"] >> 8
    assert differ["upper_six"] and not differ["upper_six"] >> 16   # six passes skipped
    assert all((differ["distinct"] >> (8 * d)) & 0xFF for d in range(8))  # every pass runs
    assert c["extremes"].min() == 0 and c["extremes"].max() == (1 << 64) - 1
    assert np.unique(c["distinct"]).size == c["distinct"].size
    sizes = {v.size for v in c.values()}
    assert {1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 7} <= sizes
    assert c["one_key"].size > 2 * TILE  # one run over several workgroups
    digits = lambda k: {d for d in range(8) if (differ[k] >> (8 * d)) & 0xFF}  # noqa: E731
    assert digits("digits_0_3_7") == {0, 3, 7}  # passes on digits that are not neighbours
    assert digits("digits_1_2_4_5_6") == {1, 2, 4, 5, 6}
    for k in ("nine_tiles_plus_5", "seventeen_tiles_plus_3"):
        tiles = -(-c[k].size // TILE)
        assert tiles >= 9 and tiles % 8 and len(digits(k)) == 8  # the tile order is permuted
    assert {9 * TILE + 5, 17 * TILE + 3} <= sizes


def test_constants_mirror_the_kernel_source():
    """worker_ref.py sizes the seam case by copies of the constants of
    psg_sort.h (the sort and the scans) and psg_worker.hip (the rest); a
    change there must change them here.  Each is defined once across the two."""
    csrc = os.path.join(ROOT, "parameter_server_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in ("psg_sort.h", "psg_worker.hip"))

    def number(pattern):
        found = re.findall(pattern, src, flags=re.M)
        assert len(found) == 1, (pattern, found)
        return int(found[0])

    assert number(r"^#define PSG_SORT_KPT (\d+)\b") == R.SORT_KPT
    assert number(r"^#define PSG_LONG_RUN (\d+)\b") == R.LONG_RUN
    assert number(r"^#define PSG_CHAIN_AHEAD (\d+)\b") * 64 == R.CHAIN
    assert number(r"^#define PSG_CHAIN_AHEAD2 (\d+)\b") * 64 == R.CHAIN2
    assert number(r"^constexpr uint32_t kFlagTile = (\d+);") == R.FLAG_TILE
    assert number(r"^constexpr uint32_t kLongGrid = (\d+);") == R.LONG_GRID
    # what the mirrors stand for in the source
    def once(pattern):
        return len(re.findall(pattern, src, flags=re.M)) == 1

    assert once(r"^constexpr uint32_t kSortTile = 256 \* kSortKPT;")
    assert once(r"^constexpr uint32_t kLongRun = PSG_LONG_RUN;")
    assert once(r"^constexpr int kChainAhead = PSG_CHAIN_AHEAD;")
    assert once(r"^constexpr int kChainAhead2 = PSG_CHAIN_AHEAD2;")
    # row_scan_kernel's trips and objv_kernel's
    assert src.count("for (uint32_t b = 0; b < n; b += %d)" % R.SCAN) == 1
    assert src.count("for (uint32_t p = threadIdx.x; p < nparts; p += %d)" % R.SCAN) == 1
    assert _lib.lib().psg_mb_sort_tile() == 256 * R.SORT_KPT


SEAM_SEED = 29


def seam_tile():
    return int(_lib.lib().psg_mb_sort_tile())


def test_seam_case_reaches_every_second_level_path():
    """The table of what no small case reaches, as assertions: a change to a
    constant or to the generator cannot quietly empty the seam case."""
    tile = seam_tile()
    offset, index, value, y = R.seam_case(tile, SEAM_SEED)
    dic = R.seam_dict(index)
    rep = R.seam_report(offset, index, dic, tile)
    print({k: v for k, v in rep.items() if k != "dict_run_lengths"})
    assert rep["pairs"] == (R.SCAN + 1) * max(tile, R.FLAG_TILE) + 1 < 1 << 20
    assert rep["rows"] == 256 * 256 + 301 and rep["empty_rows"] == [0, 7, 8, 1]
    # row_scan_kernel goes round again, with a carry; xcd_index permutes
    assert rep["sort_tiles"] > R.SCAN and rep["sort_tiles"] % 8
    assert rep["flag_tiles"] > R.SCAN and rep["flag_tiles"] % 8
    assert rep["differing_digits"] == 8 and rep["carry_passes"]
    assert rep["heads_before"] and rep["heads_after"]
    assert rep["kept_before"] and rep["kept_after"]
    assert rep["dropped_before"] and rep["dropped_after"]
    # the long-run kernels' waves go round again; a long run is dropped, too
    assert rep["long_dict_keys"] > 4 * R.LONG_GRID and rep["long_dropped"]
    # objv_kernel goes round again
    assert rep["loss_partials"] > R.SCAN
    # the short / long split and chain_sum's batches at their edges
    assert set(R.SEAM_EDGE_RUNS) <= rep["dict_run_lengths"]
    assert {R.LONG_RUN, R.LONG_RUN + 1, R.CHAIN - 1, R.CHAIN, R.CHAIN + 1, 2 * R.CHAIN,
            2 * R.CHAIN + 1} <= set(R.SEAM_EDGE_RUNS)
    assert set(range(1, 9)) <= rep["dict_run_lengths"] and rep["dict_absent"] >= 50
    assert dic[0] < index.min() and dic[-1] > index.max()
    assert np.all(dic[1:] > dic[:-1])
    # the binary case is the same structure without values
    ob, ib, vb, yb = R.seam_case(tile, SEAM_SEED, binary=True)
    assert vb is None and np.array_equal(ib, index) and np.array_equal(ob, offset)
    # the small case of the run edges
    o, i, v, yy, d = R.run_edge_case()
    st = R.Step("vector", o, i, v, yy, d)
    assert sorted(st.cnt.tolist()) == sorted(R.RUN_EDGES) and 4000 < i.size < 6000
    assert not np.array_equal(st.cnt, np.sort(st.cnt))  # key order is not length order
    assert int(np.sum(st.pos + st.neg == 0)) == 2 == d.size - st.uniq.size


def test_seam_case_sums_are_order_sensitive():
    """test_order_sensitivity_guard's bar on the seam case: reversing a run of
    8 or more (a row of 8 or more) changes at least 30 % of the outputs."""
    offset, index, value, y = R.seam_case(seam_tile(), SEAM_SEED)
    dic = R.seam_dict(index)
    st = R.Step("vector", offset, index, value, y, dic)
    rng = np.random.default_rng(2)
    x, c = R.special_vector(rng, dic.size), R.special_vector(rng, y.size)
    fwd = R.scalar_times(st.new_offset, st.new_index, st.new_value, x)
    bwd = R.scalar_times(st.new_offset, st.new_index, st.new_value, x, reverse=True)
    long_rows = np.diff(st.new_offset.astype(np.int64)) >= 8
    frac = np.mean(R.bits(fwd)[long_rows] != R.bits(bwd)[long_rows])
    print("times: %d rows of 8 or more, %.0f %% change" % (long_rows.sum(), 100 * frac))
    assert long_rows.sum() >= 1000 and frac >= 0.30
    gf = R.scalar_trans_times(st.new_offset, st.new_index, st.new_value, c, dic.size)
    gb = R.scalar_trans_times(st.new_offset, st.new_index, st.new_value, c, dic.size,
                              reverse=True)
    long_runs = (st.pos + st.neg) >= 8
    frac = np.mean(R.bits(gf)[long_runs] != R.bits(gb)[long_runs])
    print("trans_times: %d runs of 8 or more, %.0f %% change" % (long_runs.sum(), 100 * frac))
    assert long_runs.sum() > 4 * R.LONG_GRID and frac >= 0.30
    edge = np.isin(st.pos + st.neg, R.SEAM_EDGE_RUNS[2:])  # 64 and up: one key each
    assert edge.sum() == len(R.SEAM_EDGE_RUNS) - 2
    assert np.mean(R.bits(gf)[edge] != R.bits(gb)[edge]) >= 0.30


@pytest.mark.parametrize("binary", (False, True))
def test_forms_agree_on_a_cut_down_seam_case(binary):
    """The same generator with fewer pairs, so that the scalar form finishes
    in seconds; every kind of run is still there."""
    offset, index, value, y = R.seam_case(seam_tile(), SEAM_SEED, binary=binary, n=120000,
                                          rows=16000, long_keys=800)
    dic = R.seam_dict(index)
    w = np.random.default_rng(5).standard_normal(dic.size) * 2.0 ** -19
    st = both(offset, index, value, y, dic, w)
    assert set(R.SEAM_EDGE_RUNS) <= set((st.pos + st.neg).tolist())
    assert np.isfinite(st.loss).all() and np.any(st.remapped == 0)


def test_cases_take_every_branch():
    """As test_parity_case_takes_every_bookkeeping_branch does for FTRL."""
    seen = {}
    for binary in (False, True):
        offset, index, value, y = R.zipf_case(binary=binary)
        for dname, dic in R.dict_cases(np.unique(index)).items():
            rep = R.branch_report(offset, index, value, dic)
            for k, v in rep.items():
                seen[k] = seen.get(k, False) or v
            if dname == "all":
                assert not rep["dropped"] and rep["id_twice_in_row"]
            if dname == "every_other":
                assert rep["dropped"] and rep["kept"] and rep["emptied_by_dict"]
            if dname == "with_absent":
                assert rep["dict_below_min"] and rep["dict_above_max"] and \
                    rep["dict_absent_inside"]
            if dname == "empty":
                assert not rep["kept"]
            assert rep["empty_first"] and rep["empty_last"] and rep["empty_consecutive"]
            assert rep["run_over_wave"]
    assert all(seen.values()), seen
    y = R.zipf_case(kinds=R.ODD_LABELS)[3]
    assert np.isnan(y).any() and (y == 2.5).any() and (y == -1).any() and (y == 1).any()
    assert (R.bits(y) == R.bits(np.array([-0.0]))[0]).any() and (R.bits(y) == 0).any()
    offset, index, _, _ = R.column_case()
    assert np.unique(index, return_counts=True)[1].max() == 2000 == offset.size - 1


def test_order_sensitivity_guard():
    """Summing a row or a run backwards must change the bits of at least 30 %
    of the outputs of length >= 8: otherwise the bit-exact GPU tests could
    not tell an ordered sum from an unordered one.  Measured on the CPU:
    51 % at length 8, 87 % at 64, 96 % at 700."""
    rng = np.random.default_rng(2)
    for length, rows in ((8, 400), (64, 200), (700, 40)):
        n = length * rows
        offset = (np.arange(rows + 1) * length).astype(np.uint64)
        index = np.tile(np.arange(length, dtype=np.uint32), rows)
        value = R.sensitive_values(rng, n)
        x = R.sensitive_values(rng, length)
        fwd = R.scalar_times(offset, index, value, x)
        bwd = R.scalar_times(offset, index, value, x, reverse=True)
        frac = np.mean(R.bits(fwd) != R.bits(bwd))
        print("times: length %d: %.0f %% change" % (length, 100 * frac))
        assert frac >= 0.30, (length, frac)
        # the transpose of the same shape: `length` runs of `rows` terms each
        c = R.sensitive_values(rng, rows)
        gf = R.scalar_trans_times(offset, index, value, c, length)
        gb = R.scalar_trans_times(offset, index, value, c, length, reverse=True)
        if rows >= 8:
            frac = np.mean(R.bits(gf) != R.bits(gb))
            print("trans_times: runs of %d: %.0f %% change" % (rows, 100 * frac))
            assert frac >= 0.30, (rows, frac)
    # and on the shapes the GPU tests use
    offset, index, value, y = R.zipf_case()
    st = R.Step("scalar", offset, index, value, y, np.unique(index))
    x = R.special_vector(rng, st.pos.size)
    fwd = R.scalar_times(st.new_offset, st.new_index, st.new_value, x)
    bwd = R.scalar_times(st.new_offset, st.new_index, st.new_value, x, reverse=True)
    long_rows = np.diff(st.new_offset.astype(np.int64)) >= 8
    assert long_rows.sum() >= 50
    assert np.mean(R.bits(fwd)[long_rows] != R.bits(bwd)[long_rows]) >= 0.30
    c = R.special_vector(rng, y.size)
    gf = R.scalar_trans_times(st.new_offset, st.new_index, st.new_value, c, st.pos.size)
    gb = R.scalar_trans_times(st.new_offset, st.new_index, st.new_value, c, st.pos.size,
                              reverse=True)
    long_runs = (st.pos + st.neg) >= 8
    assert long_runs.sum() >= 20
    assert np.mean(R.bits(gf)[long_runs] != R.bits(gb)[long_runs]) >= 0.30


def test_tail_filter_case_drops_and_keeps():
    """The closed loop's first minibatch under tail_feature_freq = 2: at least
    one key occurs more than twice (kept) and one at most twice (dropped),
    whatever the filter's collisions add."""
    cnt = R.scalar_count_uniq(R.closed_loop_batches()[0][1])[3]
    assert (cnt > 2).any() and (cnt <= 2).any()


def test_library_exports_and_binds_every_mb_symbol():
    src = open(os.path.join(ROOT, "include", "psg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(psg_mb_[a-z_0-9]+)\s*\(", src)))
    for need in ("psg_mb_create", "psg_mb_destroy", "psg_mb_load", "psg_mb_uniq",
                 "psg_mb_localize", "psg_mb_times", "psg_mb_trans_times", "psg_mb_gradient",
                 "psg_mb_read"):
        assert need in names
    L = _lib.lib()
    for n in names:
        assert n in _lib.SIGNATURES and C.cast(getattr(L, n), C.c_void_p).value, n
    assert L.psg_mb_sort_tile() >= 256
    # argument checks that need no device
    assert L.psg_mb_create(None, C.byref(C.c_void_p())) == _lib.PSG_ERR_ARG
    assert L.psg_mb_load(None, None, 0, None, None, None) == _lib.PSG_ERR_ARG
    n = C.c_size_t()
    assert L.psg_mb_uniq(None, None, None, C.byref(n)) == _lib.PSG_ERR_ARG
    assert L.psg_mb_gradient(None, 0, None, None, None, None) == _lib.PSG_ERR_ARG


def test_worker_module_imports():
    import parameter_server_amd
    from parameter_server_amd import worker
    assert parameter_server_amd.FTRLWorker is worker.FTRLWorker
    assert parameter_server_amd.Minibatch is worker.Minibatch
    assert set(worker.ARRAYS) >= {"sorted_key", "sorted_pos", "uniq_key", "key_cnt", "new_offset",
                                  "new_index", "new_value", "pos", "neg", "xw", "tau", "loss",
                                  "grad"}
