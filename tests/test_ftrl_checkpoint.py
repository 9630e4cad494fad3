"""CPU: the host side of the FTRL checkpoint -- the model-file parse
(``read_model_text``, the first half of ModelEvaluation::run), the ``.npz``
image format, and the argument validation of the new entry points, none of
which touches a device."""
import ctypes as C

import numpy as np
import pytest

import ftrl_ref as R
from parameter_server_amd import _lib
from parameter_server_amd.ftrl import (STATE_VERSION, load_state, read_model_text, save_state)


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def same(keys, w, want):
    """(keys, w) is the sorted map `want` = {key: weight}, by bits."""
    ks = sorted(want)
    assert keys.dtype == np.uint64 and w.dtype == np.float64
    assert keys.tolist() == ks
    assert R.bits(w).tolist() == R.bits([want[k] for k in ks]).tolist()


# ---------------------------------------------------------- read_model_text --
def test_last_pair_wins_within_a_file(tmp_path):
    p = write(tmp_path, "m", "5\t1.5\n3\t-2\n5\t0.25\n9\t7\n3\t4\n")
    same(*read_model_text(p), {3: 4.0, 5: 0.25, 9: 7.0})


def test_later_files_override_earlier_ones(tmp_path):
    a = write(tmp_path, "a", "1\t1\n2\t2\n3\t3\n")
    b = write(tmp_path, "b", "2\t20\n4\t40\n")
    c = write(tmp_path, "c", "4\t-0\n1\t100\n")
    same(*read_model_text([a, b, c]), {1: 100.0, 2: 20.0, 3: 3.0, 4: -0.0})
    same(*read_model_text([c, b, a]), {1: 1.0, 2: 2.0, 3: 3.0, 4: 40.0})


def test_blank_lines_and_mixed_whitespace(tmp_path):
    # `in >> k >> v` skips any whitespace: pairs may share a line or span two
    p = write(tmp_path, "m", "\n\n  7 \t 1e-3\r\n\n8\n2.5   9 -1\n\t\n18446744073709551615\t3\n\n")
    same(*read_model_text(p), {7: 1e-3, 8: 2.5, 9: -1.0, (1 << 64) - 1: 3.0})


def test_float32_rounds_each_weight_through_float(tmp_path):
    vals = [0.1, -1.234567, 3.4e38, 1e-45, 16777217.0, 0.333333]
    p = write(tmp_path, "m", "".join("%d\t%r\n" % (i + 1, v) for i, v in enumerate(vals)))
    k64, w64 = read_model_text(p)
    k32, w32 = read_model_text(p, real=np.float32)
    assert k64.tolist() == k32.tolist() == list(range(1, len(vals) + 1))
    assert R.bits(w64).tolist() == R.bits(vals).tolist()
    want = np.array(vals, np.float64).astype(np.float32).astype(np.float64)
    assert R.bits(w32).tolist() == R.bits(want).tolist()
    assert (w32 != w64).sum() >= 4          # the rounding is visible
    with pytest.raises(ValueError):
        read_model_text(p, real=np.float16)


def test_unpaired_token_is_an_error(tmp_path):
    with pytest.raises(ValueError, match="without a value"):
        read_model_text(write(tmp_path, "m", "1\t2\n3\n"))
    with pytest.raises(ValueError, match="uint64"):
        read_model_text(write(tmp_path, "k", "1\t2\nx\t3\n"))
    with pytest.raises(ValueError, match="uint64"):
        read_model_text(write(tmp_path, "big", "18446744073709551616\t3\n"))
    with pytest.raises(ValueError, match="number"):
        read_model_text(write(tmp_path, "v", "1\ttwo\n"))


def test_no_phantom_key_zero(tmp_path):
    # the reference's loop assigns weight[0] after the last line; we do not
    p = write(tmp_path, "m", "4\t1\n6\t2\n")
    keys, _ = read_model_text(p)
    assert keys.tolist() == [4, 6]
    e = write(tmp_path, "empty", "")
    keys, w = read_model_text(e)
    assert keys.size == 0 and w.size == 0 and keys.dtype == np.uint64
    # a real key 0 is read like any other
    same(*read_model_text(write(tmp_path, "z", "0\t9\n4\t1\n")), {0: 9.0, 4: 1.0})


def test_round_trip_through_the_restated_dump(tmp_path):
    uni, msgs = R.parity_case(seed=3, nmsg=3, n=300, universe=500)
    ref = R.VectorFTRL(**R.PARITY_PARAM)
    for m in msgs:
        ref.push(*m)
    text = R.dump_text(ref, uni)
    assert text.count("\n") == ref.nnz > 100
    keys, w = read_model_text(write(tmp_path, "dump", text))
    k, v = R.nonzero(ref, uni)
    assert keys.tolist() == k.tolist()
    want = [float("%g" % x) for x in v.tolist()]     # what the dump's 6 digits keep
    assert R.bits(w).tolist() == R.bits(want).tolist()
    _, w32 = read_model_text(write(tmp_path, "dump32", text), real=np.float32)
    assert R.bits(w32).tolist() == R.bits(np.array(want).astype(np.float32)
                                          .astype(np.float64)).tolist()


# -------------------------------------------------------------- .npz format --
def image():
    nan = np.array([0x7ff8000000000123, 0xfff0000000000001], np.uint64).view(np.float64)
    keys = np.array([0, 1, 77, 1 << 63, (1 << 64) - 1], np.uint64)
    pos = np.array([0, (1 << 32) + 5, 3, (1 << 64) - 1, 9], np.uint64)
    neg = np.array([1, 2, 1 << 40, 0, 4], np.uint64)
    w = np.array([-0.0, 0.0, nan[0], 1.5, -2.25])
    z = np.array([nan[1], -0.0, 4.0, np.inf, -1e-310])
    return keys, pos, neg, w, z


def test_npz_round_trip_by_bits(tmp_path):
    arrays = image()
    param = np.array([0x3fb999999999999a, 0x7ff8000000000abc, 0x8000000000000000,
                      0x3ff0000000000001], np.uint64).view(np.float64)
    path = str(tmp_path / "model.ckpt")      # exactly this path: no suffix is added
    save_state(path, *arrays, *param.tolist(), frozen=True, objv=np.array(2.5),
               table=np.arange(70, dtype=np.uint8))
    st = load_state(path)
    for name, a in zip(("keys", "pos", "neg", "w", "z"), arrays):
        assert st[name].dtype == a.dtype
        assert st[name].view(np.uint64).tolist() == a.view(np.uint64).tolist(), name
    for name, v in zip(("alpha", "beta", "lambda1", "lambda2"), param):
        assert st[name].dtype == np.float64
        assert R.bits(float(st[name])).tolist() == R.bits(v).tolist(), name
    assert int(st["frozen"]) == 1 and int(st["format_version"]) == STATE_VERSION
    assert float(st["objv"]) == 2.5 and st["table"].tolist() == list(range(70))
    # an empty model is an image too
    empty = [a[:0] for a in arrays]
    save_state(path, *empty, 1.0, 1.0, 0.0, 0.0)
    st = load_state(path)
    assert st["keys"].size == 0 and st["keys"].dtype == np.uint64 and int(st["frozen"]) == 0


def test_npz_rejects_an_unknown_version_and_bad_shapes(tmp_path):
    arrays = image()
    path = str(tmp_path / "model.npz")
    save_state(path, *arrays, 1.0, 1.0, 0.0, 0.0)
    with np.load(path) as f:
        fields = {k: f[k] for k in f.files}
    fields["format_version"] = np.array(STATE_VERSION + 1, np.int64)
    np.savez(path, **fields)
    with pytest.raises(ValueError, match="version"):
        load_state(path)
    del fields["format_version"]
    np.savez(path, **fields)
    with pytest.raises(ValueError, match="version"):
        load_state(path)
    with pytest.raises(ValueError):
        save_state(path, arrays[0], arrays[1][:-1], *arrays[2:], 1.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        save_state(path, *arrays, 1.0, 1.0, 0.0, 0.0, format_version=np.zeros(1))


# ------------------------------------------------------ argument validation --
def test_new_entry_points_validate_before_touching_a_context():
    L = _lib.lib()
    ARG = _lib.PSG_ERR_ARG
    k = np.array([1, 2], np.uint64)
    c = np.array([1, 2], np.uint64)
    w = np.array([1.0, 2.0])
    n, nd, fz = C.c_size_t(), C.c_uint64(), C.c_int()
    table = np.zeros(64, np.uint8)
    p = lambda a: a.ctypes.data
    # a null context
    assert L.psg_ftrl_import(None, p(k), 2, p(c), p(c), p(w), p(w)) == ARG
    assert L.psg_ftrl_import_dev(None, p(k), 2, p(c), p(c), p(w), p(w), None) == ARG
    assert L.psg_ftrl_export_state(None, None, None, None, None, None, None, 0, C.byref(n)) == ARG
    assert L.psg_ftrl_export_state_dev(None, None, None, None, None, None, None, 0,
                                       C.addressof(nd), None) == ARG
    assert L.psg_ftrl_frozen(None, C.byref(fz)) == ARG
    assert L.psg_freq_table_assign(None, 0, p(table), 64) == ARG
    # null arrays with n > 0, a null count, a partly null form, an inverted
    # range: all refused before the context is looked at (any non-null
    # address stands for it here)
    ctx = C.create_string_buffer(1 << 16)
    for f in (L.psg_ftrl_import, L.psg_ftrl_import_dev):
        tail = [None] if f is L.psg_ftrl_import_dev else []
        assert f(ctx, None, 2, p(c), p(c), p(w), p(w), *tail) == ARG
        assert f(ctx, p(k), 2, p(c), p(c), None, p(w), *tail) == ARG
        assert f(ctx, p(k), 2, None, None, None, None, *tail) == ARG
        for form in ((None, p(c), p(w)), (p(c), None, p(w)), (p(c), p(c), None),
                     (None, None, p(w)), (p(c), None, None)):
            assert f(ctx, p(k), 2, form[0], form[1], p(w), form[2], *tail) == ARG
            assert b"all given or all NULL" in L.psg_last_error()
    assert L.psg_ftrl_export_state(ctx, None, None, None, None, None, None, 0, None) == ARG
    assert L.psg_ftrl_export_state_dev(ctx, None, None, None, None, None, None, 0, None,
                                       None) == ARG
    bad = (C.c_uint64 * 2)(5, 4)
    assert L.psg_ftrl_export_state(ctx, bad, None, None, None, None, None, 0, C.byref(n)) == ARG
    assert L.psg_ftrl_export_state_dev(ctx, bad, None, None, None, None, None, 0,
                                       C.addressof(nd), None) == ARG
    assert L.psg_ftrl_frozen(ctx, None) == ARG
    assert L.psg_freq_table_assign(ctx, 0, None, 64) == ARG
