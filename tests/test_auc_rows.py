"""CPU: the row-valued AUC's symbols and prototypes, its argument checks that
need no device, and AUCRows.accuracy / evaluate as the existing *_data
functions over each model's export."""
import ctypes as C

import numpy as np

import auc_ref as R
from parameter_server_amd import _lib
from parameter_server_amd.auc import AUCRows, accuracy_data, evaluate_data

NAMES = ("create", "destroy", "clear", "set_goodness", "add_dev", "add", "merge", "data",
         "accuracy", "evaluate")


def test_symbols_are_exported_with_the_declared_prototypes():
    L, raw = _lib.lib(), C.CDLL(_lib.LIB_PATH)
    for name in ["psg_auc_rows_" + n for n in NAMES] + ["psg_mb_rows_labels"]:
        restype, argtypes = _lib.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
        assert C.cast(getattr(raw, name), C.c_void_p).value
    # model-indexed calls take j right after the handle
    assert _lib.SIGNATURES["psg_auc_rows_data"][1][1] is C.c_int
    assert _lib.SIGNATURES["psg_auc_rows_merge"][1][1] is C.c_int


def test_null_arguments_need_no_device():
    L = _lib.lib()
    v = (C.c_double * 2)()
    nt = C.c_size_t()
    assert L.psg_auc_rows_create(None, 10, 2, C.byref(C.c_void_p())) == _lib.PSG_ERR_ARG
    assert L.psg_auc_rows_clear(None) == _lib.PSG_ERR_ARG
    assert L.psg_auc_rows_set_goodness(None, 10) == _lib.PSG_ERR_ARG
    assert L.psg_auc_rows_add_dev(None, None, None, 0, None) == _lib.PSG_ERR_ARG
    assert L.psg_auc_rows_add(None, None, None, 0) == _lib.PSG_ERR_ARG
    assert L.psg_auc_rows_merge(None, 0, None, None, 0, None, None, 0) == _lib.PSG_ERR_ARG
    assert L.psg_auc_rows_data(None, 0, None, None, 0, C.byref(nt), None, None, 0,
                               C.byref(nt)) == _lib.PSG_ERR_ARG
    assert L.psg_auc_rows_accuracy(None, 0.0, v) == _lib.PSG_ERR_ARG
    assert L.psg_auc_rows_evaluate(None, 0, v) == _lib.PSG_ERR_ARG
    L.psg_auc_rows_destroy(None)


def test_accuracy_and_evaluate_reduce_to_the_data_functions():
    rng = np.random.default_rng(3)
    g = 10
    datas = [R.vector_compute(R.mixed_labels(rng, 500), rng.normal(0, 3, 500), g) for _ in range(3)]
    a = AUCRows.__new__(AUCRows)  # no handle: the export is given
    a._h, a.m, a.goodness, a.data = None, 3, g, lambda j: datas[j]
    for th in (0.0, 0.5):
        assert np.array_equal(R.bits(a.accuracy(th)),
                              R.bits([accuracy_data(g, *d, threshold=th) for d in datas]))
        assert np.array_equal(R.bits(a.accuracy(th)),
                              R.bits([R.vector_accuracy(d, g, th) for d in datas]))
    for w in (False, True):
        assert np.array_equal(R.bits(a.evaluate(w)),
                              R.bits([evaluate_data(*d, as_written=w) for d in datas]))
        assert np.array_equal(R.bits(a.evaluate(w)),
                              R.bits([R.vector_evaluate(d, w) for d in datas]))
