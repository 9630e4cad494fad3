"""Python mirror of the reference's online worker step over the C ABI.

``Minibatch`` is a thin class over ``psg_mb_*`` (include/psg.h): one worker
minibatch resident in HBM, with ``Localizer::countUniqIndex`` / ``remapIndex``
(reference src/base/localizer.h:50-168), ``FTRL::countKeys``
(src/linear_method/ftrl.cc:154-174), ``Xw = Z * w``, ``LogitLoss``
(src/linear_method/loss.h:73-85) and the gradient as device kernels.

``FTRLWorker.step`` is the body of ``FTRL::updateModel``'s loop
(ftrl.cc:88-151) against an ``FTRLModel`` in the same context: unique keys,
tail filter, pull, localize, gradient, push.  Every array stays on the
device between those calls; the host reads ``n_uniq``, the filter's kept
count and ``objv``, the three points at which the reference worker waits
(ftrl.cc:102,122,130).
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from . import _lib
from .auc import exact_auc
from .ftrl import FTRLModel, load_state
from .kv_vector import _ptr

# psg_mb_read's arrays: name -> (id, dtype)
ARRAYS = {
    "sorted_key": (_lib.PSG_MB_SORTED_KEY, np.uint64),
    "sorted_pos": (_lib.PSG_MB_SORTED_POS, np.uint32),
    "uniq_key": (_lib.PSG_MB_UNIQ_KEY, np.uint64),
    "key_cnt": (_lib.PSG_MB_KEY_CNT, np.uint32),
    "new_offset": (_lib.PSG_MB_NEW_OFFSET, np.uint64),
    "new_index": (_lib.PSG_MB_NEW_INDEX, np.uint32),
    "new_value": (_lib.PSG_MB_NEW_VALUE, np.float64),
    "pos": (_lib.PSG_MB_POS, np.uint32),
    "neg": (_lib.PSG_MB_NEG, np.uint32),
    "xw": (_lib.PSG_MB_XW, np.float64),
    "tau": (_lib.PSG_MB_TAU, np.float64),
    "loss": (_lib.PSG_MB_LOSS, np.float64),
    "grad": (_lib.PSG_MB_GRAD, np.float64),
    "run_start": (_lib.PSG_MB_RUN_START, np.uint32),
    "remapped": (_lib.PSG_MB_REMAPPED, np.uint32),
    "row_of": (_lib.PSG_MB_ROW_OF, np.uint32),
    "offset": (_lib.PSG_MB_OFFSET, np.uint64),
    "index": (_lib.PSG_MB_INDEX, np.uint64),
    "value": (_lib.PSG_MB_VALUE, np.float64),
    "y": (_lib.PSG_MB_Y, np.float64),
    "slot": (_lib.PSG_MB_SLOT, np.uint16),
}
FORMATS = {"adfea": _lib.PSG_TEXT_ADFEA, "libsvm": _lib.PSG_TEXT_LIBSVM}


def text_chunk() -> int:
    """Bytes of text per workgroup of the ingest kernels (psg_text_chunk)."""
    return int(_lib.lib().psg_text_chunk())


def _format(fmt) -> int:
    return FORMATS[fmt] if isinstance(fmt, str) else int(fmt)


def parse_text_host(text: bytes, fmt, max_rows=None, final: bool = True):
    """psg_text_parse_host: (offset, index, value or None, y, result), parsed
    serially on the host; what ``Minibatch.load_text`` loads."""
    L = _lib.lib()
    text = bytes(text)
    f = _format(fmt)
    cap = (1 << 64) - 1 if max_rows is None else int(max_rows)
    r = _lib.TextResult()
    _lib.check(L.psg_text_parse_host(text, len(text), f, cap, 1 if final else 0, None, None, None,
                                     None, 0, 0, C.byref(r)))
    offset = np.zeros(r.rows + 1, np.uint64)
    index = np.zeros(r.nnz, np.uint64)
    value = np.zeros(r.nnz, np.float64) if f == _lib.PSG_TEXT_LIBSVM else None
    y = np.zeros(r.rows, np.float64)
    _lib.check(L.psg_text_parse_host(text, len(text), f, cap, 1 if final else 0, _ptr(offset),
                                     _ptr(index), _ptr(value) if value is not None else None,
                                     _ptr(y), int(r.rows), int(r.nnz), C.byref(r)))
    return offset, index, value, y, r


def sort_tile() -> int:
    """Pairs per workgroup of the device sort (psg_mb_sort_tile)."""
    return int(_lib.lib().psg_mb_sort_tile())


class Minibatch:
    """One worker minibatch (row-major CSR with global ids) on the device of
    context ``ctx`` (a ``psg_ctx`` handle of a PSG_F64 context)."""

    def __init__(self, ctx):
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.psg_mb_create(ctx, C.byref(h)))
        self._h = h
        self.rows = self.nnz = self.n_uniq = self.ndict = 0
        s = C.c_void_p()
        _lib.check(self._L.psg_mb_stream(h, C.byref(s)))
        self.stream = s.value  # the context's
        self.uniq_key_dev = self.key_cnt_dev = None
        self.pos_dev = self.neg_dev = self.grad_dev = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.psg_mb_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def load(self, offset, index, value, y) -> None:
        """psg_mb_load; ``value`` None: a binary matrix."""
        offset = np.ascontiguousarray(offset, dtype=np.uint64)
        index = np.ascontiguousarray(index, dtype=np.uint64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if offset.size < 1 or y.size != offset.size - 1:
            raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{y.size} labels for {offset.size} offsets")
        if value is not None:
            value = np.ascontiguousarray(value, dtype=np.float64)
            if value.size != index.size:  # CHECK_EQ(value.size(), index.size()) localizer.h:119
                raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{value.size} values, {index.size} ids")
        if int(offset[-1]) < (1 << 32) - 1 and int(offset[-1]) != index.size:
            raise _lib.PSGError(_lib.PSG_ERR_SIZE,  # CHECK_EQ(offset.back(), index.size()) :116
                                f"offset ends at {int(offset[-1])}, {index.size} ids")
        _lib.check(self._L.psg_mb_load(self._h, _ptr(offset), offset.size - 1, _ptr(index),
                                       _ptr(value) if value is not None else None, _ptr(y)))
        self.rows, self.nnz = offset.size - 1, index.size
        self.n_uniq = self.ndict = 0

    def load_text(self, text: bytes, fmt, max_rows=None, final: bool = True):
        """psg_mb_load_text: LIBSVM / ADFEA lines (``fmt``: "libsvm", "adfea"
        or a PSG_TEXT_* id) parsed on the device into this minibatch.  Returns
        the psg_text_result: rows, nnz, consumed, bad_line, slow_tokens,
        parse_ms."""
        text = bytes(text) if not isinstance(text, bytes) else text
        cap = (1 << 64) - 1 if max_rows is None else int(max_rows)
        r = _lib.TextResult()
        _lib.check(self._L.psg_mb_load_text(self._h, text, len(text), _format(fmt), cap,
                                            1 if final else 0, C.byref(r)))
        self.rows, self.nnz = int(r.rows), int(r.nnz)
        self.n_uniq = self.ndict = 0
        return r

    def load_text_groups(self, text: bytes, fmt, max_rows=None, final: bool = True):
        """psg_mb_load_text_groups: ``load_text`` by the grouped parse's line
        rule, with the slot id of every entry resident too (read("slot"))."""
        text = bytes(text) if not isinstance(text, bytes) else text
        cap = (1 << 64) - 1 if max_rows is None else int(max_rows)
        r = _lib.TextResult()
        _lib.check(self._L.psg_mb_load_text_groups(self._h, text, len(text), _format(fmt), cap,
                                                   1 if final else 0, C.byref(r)))
        self.rows, self.nnz = int(r.rows), int(r.nnz)
        self.n_uniq = self.ndict = 0
        return r

    def uniq(self) -> int:
        """psg_mb_uniq: n_uniq; the device arrays are uniq_key_dev, key_cnt_dev."""
        k, c, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        _lib.check(self._L.psg_mb_uniq(self._h, C.byref(k), C.byref(c), C.byref(n)))
        self.uniq_key_dev, self.key_cnt_dev, self.n_uniq = k.value, c.value, n.value
        return n.value

    def localize(self, dict_dev, ndict: int, stream=None) -> None:
        """psg_mb_localize against ndict device keys; pos_dev / neg_dev."""
        p, q = C.c_void_p(), C.c_void_p()
        _lib.check(self._L.psg_mb_localize(self._h, dict_dev, ndict, C.byref(p), C.byref(q),
                                           stream))
        self.pos_dev, self.neg_dev, self.ndict = p.value, q.value, ndict

    def times(self, x_dev, xw_dev, stream=None) -> None:
        _lib.check(self._L.psg_mb_times(self._h, x_dev, xw_dev, stream))

    def labels(self) -> Tuple[int, int]:
        """psg_mb_labels: the device pointers of y and of the minibatch's Xw."""
        y, xw = C.c_void_p(), C.c_void_p()
        _lib.check(self._L.psg_mb_labels(self._h, C.byref(y), C.byref(xw)))
        return y.value, xw.value

    def trans_times(self, c_dev, g_dev, stream=None) -> None:
        _lib.check(self._L.psg_mb_trans_times(self._h, c_dev, g_dev, stream))

    def gradient(self, w_dev, loss: int = _lib.PSG_LOSS_LOGIT, stream=None) -> float:
        """psg_mb_gradient: objv; the device gradient is grad_dev."""
        g, objv = C.c_void_p(), C.c_double()
        _lib.check(self._L.psg_mb_gradient(self._h, loss, w_dev, C.byref(g), C.byref(objv),
                                           stream))
        self.grad_dev = g.value
        return objv.value

    def scratch(self, slot: int, nbytes: int) -> int:
        """A device block of the minibatch's (psg_mb_scratch)."""
        p = C.c_void_p()
        _lib.check(self._L.psg_mb_scratch(self._h, slot, nbytes, C.byref(p)))
        return p.value

    def profile(self, on: bool = True) -> None:
        """Stage timing on or off (psg_mb_profile)."""
        _lib.check(self._L.psg_mb_profile(self._h, 1 if on else 0))

    def stage_ms(self) -> dict:
        """The last run's time of each stage in ms (psg_mb_stage_ms); waits."""
        ms = (C.c_double * len(_lib.MB_STAGES))()
        _lib.check(self._L.psg_mb_stage_ms(self._h, ms))
        return dict(zip(_lib.MB_STAGES, list(ms)))

    def _read(self, what: int, dtype) -> np.ndarray:
        n = C.c_size_t()
        rc = self._L.psg_mb_read(self._h, what, None, 0, C.byref(n))
        if rc not in (_lib.PSG_OK, _lib.PSG_ERR_SIZE):
            _lib.check(rc)
        out = np.empty(n.value, dtype)
        if n.value:
            _lib.check(self._L.psg_mb_read(self._h, what, _ptr(out), out.nbytes, C.byref(n)))
        return out

    def read(self, name: str) -> np.ndarray:
        """A host copy of one internal array (ARRAYS)."""
        what, dtype = ARRAYS[name]
        return self._read(what, dtype)

    def read_scratch(self, slot: int, dtype, count: int) -> np.ndarray:
        """The first `count` items of a scratch block, as `dtype` (8 bytes wide)."""
        a = self._read(_lib.PSG_MB_SCRATCH + slot, np.uint64)
        return a[:count].view(dtype)


class FTRLWorker:
    """The worker of the online solver (ftrl.cc:88-151) for one model.

    ``tail_feature_freq`` > 0 turns the tail filter on: a minibatch's keys
    are inserted with their counts and only those whose estimate exceeds it
    are kept (shared_parameter.h:114-133), in a CountMin of ``countmin_n``
    counters and ``countmin_k`` probes on channel ``chl`` of the context."""

    _DICT, _W, _FILTER, _WORD = 0, 1, 2, 3  # scratch slots

    def __init__(self, model: FTRLModel, tail_feature_freq: int = 0, countmin_n: int = 1 << 20,
                 countmin_k: int = 2, chl: int = 0):
        self._L = _lib.lib()
        self.model = model
        self._ctx = model._model()
        self.freq = int(tail_feature_freq)
        self.chl = chl
        # CountMin::resize's n_ and k_ (countmin.h:14-19)
        self.countmin_n = max(int(countmin_n), 64)
        self.countmin_k = min(30, max(1, int(countmin_k)))
        if self.freq > 0:
            _lib.check(self._L.psg_freq_resize(self._ctx, chl, countmin_n, countmin_k))
        self.mb = Minibatch(self._ctx)
        self.objv = 0.0   # status_.objv
        self.num_ex = 0   # status_.num_ex
        self.ndict = 0
        self.dict_dev = self.w_dev = None

    def close(self):
        self.mb.close()

    def predict(self, offset, index, value, y) -> int:
        """Score one minibatch against the model without training on it
        (ModelEvaluation::run, model_evaluation.h:48-57): the device pointer
        of Xw[rows], also ``mb.read("xw")``.  No filter insert and no push,
        and a pull does not insert: the model is left as it was."""
        self.mb.load(offset, index, value, y)
        return self._predict_loaded()

    def predict_text(self, text: bytes, fmt, max_rows=None, final: bool = True):
        """``predict`` on the next minibatch of a text buffer (``load_text``
        in place of ``load``): (the device pointer of Xw, the bytes consumed)."""
        r = self.mb.load_text(text, fmt, max_rows, final)
        return self._predict_loaded(), int(r.consumed)

    def _predict_loaded(self) -> int:
        L, mb = self._L, self.mb
        st = mb.stream
        n = mb.uniq()
        keys = mb.uniq_key_dev
        w = mb.scratch(self._W, 8 * n)
        _lib.check(L.psg_ftrl_pull_dev(self._ctx, keys, n, w, st))
        mb.localize(keys, n)
        xw = mb.labels()[1]
        mb.times(w, xw)
        self.dict_dev, self.w_dev, self.ndict = keys, w, n
        return xw

    def step(self, offset, index, value, y, auc=None) -> Tuple[float, int]:
        """One minibatch: (its objv, its number of examples).  ``auc``: an
        ``AUC`` of this context that takes (y, Xw) of the minibatch before
        the push: Xw comes from weights that have not seen the minibatch, so
        the histogram is a progressive-validation AUC."""
        self.mb.load(offset, index, value, y)
        return self._step_loaded(auc)

    def step_text(self, text: bytes, fmt, max_rows=None, final: bool = True,
                  auc=None) -> Tuple[float, int, int]:
        """``step`` on the next minibatch of a text buffer (``load_text`` in
        place of ``load``): (objv, examples, bytes consumed), so a caller walks
        a buffer minibatch by minibatch with ``text[consumed:]``."""
        r = self.mb.load_text(text, fmt, max_rows, final)
        objv, rows = self._step_loaded(auc)
        return objv, rows, int(r.consumed)

    def _step_loaded(self, auc=None) -> Tuple[float, int]:
        L, mb = self._L, self.mb
        st = mb.stream  # every enqueue of the step, in order
        n = mb.uniq()                                                      # ftrl.cc:96
        if self.freq > 0 and n:                                            # :99-106
            keys = mb.scratch(self._DICT, 8 * n)
            word = mb.scratch(self._WORD, 8)
            fs = mb.scratch(self._FILTER, L.psg_freq_query_scratch_bytes(n))
            _lib.check(L.psg_freq_insert_dev(self._ctx, self.chl, mb.uniq_key_dev,
                                             mb.key_cnt_dev, n, st))
            _lib.check(L.psg_freq_query_dev(self._ctx, self.chl, mb.uniq_key_dev, n, self.freq,
                                            keys, word, fs, st))
            ndict = int(mb.read_scratch(self._WORD, np.uint64, 1)[0])
        else:
            keys, ndict = mb.uniq_key_dev, n
        w = mb.scratch(self._W, 8 * ndict)
        _lib.check(L.psg_ftrl_pull_dev(self._ctx, keys, ndict, w, st))   # :108-111
        mb.localize(keys, ndict)                                           # :113-119
        objv = mb.gradient(w)                                              # :128-138
        if auc is not None:
            y_dev, xw_dev = mb.labels()
            auc.add_dev(y_dev, xw_dev, mb.rows, st)
        _lib.check(L.psg_ftrl_push_dev(self._ctx, keys, ndict, mb.pos_dev, mb.neg_dev,
                                       mb.grad_dev, st))                 # :141-148
        self.dict_dev, self.w_dev, self.ndict = keys, w, ndict
        self.objv += objv                                                  # :131-135
        self.num_ex += mb.rows
        return objv, mb.rows

    # -- what the last step used, for tests and checkpoints ------------------
    def last_dict(self) -> np.ndarray:
        if self.freq > 0 and self.mb.n_uniq:
            return self.mb.read_scratch(self._DICT, np.uint64, self.ndict).copy()
        return self.mb.read("uniq_key")

    def last_w(self) -> np.ndarray:
        return self.mb.read_scratch(self._W, np.float64, self.ndict).copy()

    # -- checkpoint ----------------------------------------------------------
    def freq_table(self) -> np.ndarray:
        """The tail filter's CountMin counters (psg_freq_table)."""
        out = np.zeros(self.countmin_n, np.uint8)
        _lib.check(self._L.psg_freq_table(self._ctx, self.chl, _ptr(out), out.size))
        return out

    def save(self, path) -> None:
        """Everything the next step depends on, in one ``.npz``
        (``ftrl.save_state``): the model's image and parameters, ``objv`` and
        ``num_ex``, and with the tail filter on its threshold and the CountMin
        table with its ``n`` and ``k``."""
        extra = dict(objv=np.array(self.objv, np.float64), num_ex=np.array(self.num_ex, np.int64),
                     tail_feature_freq=np.array(self.freq, np.int64))
        if self.freq > 0:
            extra.update(countmin_n=np.array(self.countmin_n, np.int64),
                         countmin_k=np.array(self.countmin_k, np.int64),
                         countmin_table=self.freq_table())
        self.model.save(path, **extra)

    @classmethod
    def load(cls, path, device: int = 0, chl: int = 0) -> "FTRLWorker":
        """A worker, with a model of its own, that goes on where ``save``
        stopped: the same steps give the same bits."""
        st = load_state(path)
        if "tail_feature_freq" not in st:
            raise ValueError(f"{path}: a model image without a worker's state")
        freq = int(st["tail_feature_freq"])
        model = FTRLModel.from_state(st, device)
        if freq > 0:
            wk = cls(model, freq, int(st["countmin_n"]), int(st["countmin_k"]), chl)
            table = np.ascontiguousarray(st["countmin_table"], dtype=np.uint8)
            _lib.check(wk._L.psg_freq_table_assign(wk._ctx, chl, _ptr(table), table.size))
        else:
            wk = cls(model, chl=chl)
        wk.objv = float(st["objv"])
        wk.num_ex = int(st["num_ex"])
        return wk


def evaluate_model(model_paths, text: bytes, fmt, max_rows: int = 100000, device: int = 0,
                   real=np.float32):
    """ModelEvaluation::run (reference src/linear_method/model_evaluation.h):
    the ``key w`` model files loaded into a frozen model (``readFromFile``;
    ``real``: the reference's ``Real`` is float), the text walked minibatch by
    minibatch of ``max_rows`` examples (:42: 100000) with ``predict_text``,
    ``y`` and ``Xw`` of each appended (:44,59), then the exact AUC of all of
    them (:66).  Returns (auc, labels, predictions).

    Defined deviation: a prediction is accumulated in double by the ordered
    product (one row's terms in the row's order), where the reference adds
    floats (``Real re``, :49-57)."""
    model = FTRLModel(device)
    wk = None
    try:
        model.readFromFile(model_paths, real=real)
        wk = FTRLWorker(model)
        text = bytes(text)
        labels, predictions = [], []
        at = 0
        while at < len(text):
            _, consumed = wk.predict_text(text[at:], fmt, max_rows)
            if wk.mb.rows:
                labels.append(wk.mb.read("y"))
                predictions.append(wk.mb.read("xw"))
            if consumed == 0:
                break
            at += consumed
        y = np.concatenate(labels) if labels else np.zeros(0, np.float64)
        xw = np.concatenate(predictions) if predictions else np.zeros(0, np.float64)
        return exact_auc(model._h, y, xw), y, xw
    finally:
        if wk is not None:
            wk.close()
        model.close()
