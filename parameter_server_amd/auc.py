"""Python mirror of the reference's evaluation over the C ABI.

``AUC`` follows ``PS::AUC`` (reference src/base/auc.h:8-103) method for
method -- ``setGoodness``, ``compute`` (here ``add`` / ``add_dev``, which also
merge), ``merge``, ``accuracy``, ``evaluate``, ``clear`` -- over the histogram
resident in HBM behind ``psg_auc_*`` (include/psg.h, which also lists the
defined deviations; the one a caller meets first: ``evaluate`` walks the
positives by KEY by default, where auc.h:49 compares their counts, and
``as_written=True`` gives the reference's own number).

``exact_auc`` is ``Evaluation<double>::auc`` (src/base/evaluation.h:17-44).
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from . import _lib
from .kv_vector import _ptr


def _lists(tp_key, tp_count, fp_key, fp_count):
    tk = np.ascontiguousarray(tp_key, dtype=np.int64)
    tc = np.ascontiguousarray(tp_count, dtype=np.uint64)
    fk = np.ascontiguousarray(fp_key, dtype=np.int64)
    fc = np.ascontiguousarray(fp_count, dtype=np.uint64)
    if tk.size != tc.size or fk.size != fc.size:  # CHECK_EQ(tp_key_size, tp_count_size) :15,19
        raise _lib.PSGError(_lib.PSG_ERR_SIZE, "AUCData: keys and counts differ in length")
    return tk, tc, fk, fc


def accuracy_data(goodness: int, tp_key, tp_count, fp_key, fp_count,
                  threshold: float = 0) -> float:
    """auc.h:26-39 over an AUCData (psg_auc_accuracy_data; no device)."""
    tk, tc, fk, fc = _lists(tp_key, tp_count, fp_key, fp_count)
    v = C.c_double()
    _lib.check(_lib.lib().psg_auc_accuracy_data(goodness, _ptr(tk), _ptr(tc), tk.size, _ptr(fk),
                                                _ptr(fc), fk.size, threshold, C.byref(v)))
    return v.value


def evaluate_data(tp_key, tp_count, fp_key, fp_count, as_written: bool = False) -> float:
    """auc.h:42-59 over an AUCData (psg_auc_evaluate_data; no device)."""
    tk, tc, fk, fc = _lists(tp_key, tp_count, fp_key, fp_count)
    v = C.c_double()
    mode = _lib.PSG_AUC_AS_WRITTEN if as_written else _lib.PSG_AUC_BY_KEY
    _lib.check(_lib.lib().psg_auc_evaluate_data(_ptr(tk), _ptr(tc), tk.size, _ptr(fk), _ptr(fc),
                                                fk.size, mode, C.byref(v)))
    return v.value


class AUC:
    """PS::AUC with its two maps resident on the device of context ``ctx``."""

    def __init__(self, ctx, goodness: int = 100000):
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.psg_auc_create(ctx, goodness, C.byref(h)))
        self._h = h
        self.goodness = int(goodness)

    def close(self):
        if getattr(self, "_h", None):
            self._L.psg_auc_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def setGoodness(self, goodness: int) -> None:
        _lib.check(self._L.psg_auc_set_goodness(self._h, goodness))
        self.goodness = int(goodness)

    def add(self, y, predict) -> None:
        """compute + merge of host arrays (psg_auc_add)."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        predict = np.ascontiguousarray(predict, dtype=np.float64)
        if y.size != predict.size:  # CHECK_EQ(label.size(), predict.size()) :70
            raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{y.size} labels, {predict.size} predictions")
        _lib.check(self._L.psg_auc_add(self._h, _ptr(y), _ptr(predict), y.size))

    def add_dev(self, y_dev, predict_dev, n: int, stream=None) -> None:
        """The same with device pointers (psg_auc_add_dev)."""
        _lib.check(self._L.psg_auc_add_dev(self._h, y_dev, predict_dev, n, stream))

    def merge(self, tp_key, tp_count, fp_key, fp_count) -> None:
        """merge(AUCData) (psg_auc_merge)."""
        tk, tc, fk, fc = _lists(tp_key, tp_count, fp_key, fp_count)
        _lib.check(self._L.psg_auc_merge(self._h, _ptr(tk), _ptr(tc), tk.size, _ptr(fk), _ptr(fc),
                                         fk.size))

    def data(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(tp_key, tp_count, fp_key, fp_count), each list ascending by key."""
        nt, nf = C.c_size_t(), C.c_size_t()
        rc = self._L.psg_auc_data(self._h, None, None, 0, C.byref(nt), None, None, 0, C.byref(nf))
        if rc not in (_lib.PSG_OK, _lib.PSG_ERR_SIZE):
            _lib.check(rc)
        tk, tc = np.empty(nt.value, np.int64), np.empty(nt.value, np.uint64)
        fk, fc = np.empty(nf.value, np.int64), np.empty(nf.value, np.uint64)
        if nt.value or nf.value:
            _lib.check(self._L.psg_auc_data(self._h, _ptr(tk), _ptr(tc), tk.size, C.byref(nt),
                                            _ptr(fk), _ptr(fc), fk.size, C.byref(nf)))
        return tk, tc, fk, fc

    def accuracy(self, threshold: float = 0) -> float:
        v = C.c_double()
        _lib.check(self._L.psg_auc_accuracy(self._h, threshold, C.byref(v)))
        return v.value

    def evaluate(self, as_written: bool = False) -> float:
        v = C.c_double()
        mode = _lib.PSG_AUC_AS_WRITTEN if as_written else _lib.PSG_AUC_BY_KEY
        _lib.check(self._L.psg_auc_evaluate(self._h, mode, C.byref(v)))
        return v.value

    def clear(self) -> None:
        _lib.check(self._L.psg_auc_clear(self._h))


def exact_auc(ctx, y, predict) -> float:
    """Evaluation<double>::auc of host arrays (psg_auc_exact)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    predict = np.ascontiguousarray(predict, dtype=np.float64)
    if y.size != predict.size:  # CHECK_EQ(n, predict.size()) evaluation.h:20
        raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{y.size} labels, {predict.size} predictions")
    v = C.c_double()
    _lib.check(_lib.lib().psg_auc_exact(ctx, _ptr(y), _ptr(predict), y.size, C.byref(v)))
    return v.value


def exact_auc_dev(ctx, y_dev, predict_dev, n: int, stream=None) -> float:
    """The same with device pointers (psg_auc_exact_dev)."""
    v = C.c_double()
    _lib.check(_lib.lib().psg_auc_exact_dev(ctx, y_dev, predict_dev, n, C.byref(v), stream))
    return v.value
