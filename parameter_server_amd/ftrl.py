"""Python mirror of the reference's online server model over the C ABI.

``FTRLModel`` follows ``PS::LM::FTRLModel<Key, double>`` (reference
src/linear_method/ftrl_model.h:12-69) method for method --
``setLearningRate``, ``setPenalty``, ``setValue``, ``getValue``, ``objv``,
``nnz``, ``writeToFile`` -- over the hash table resident in HBM behind
``psg_ftrl_*`` (include/psg.h, which also lists the defined deviations: a
pull does not insert, the norms are a reduction, a message must be strictly
increasing, the dump is sorted by key).

Checkpoint and restore fill the hooks the reference leaves empty
(``setReplica`` / ``getReplica`` / ``recoverFrom``, ftrl_model.h:41-44):
``state`` / ``restore`` move whole entries, ``save`` / ``load`` keep them in
one ``.npz``, and ``read_model_text`` / ``readFromFile`` are the model load of
``ModelEvaluation::run`` (model_evaluation.h:16-27).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import _lib
from ._lib import PSG_F64
from .kv_vector import Message, _ptr


def format_weight(w: float) -> str:
    """A double as the reference's ``out << w`` prints it (default ostream
    precision: printf %g, 6 significant digits)."""
    return "%g" % w


def read_model_text(paths, real=np.float64):
    """The model files ``ModelEvaluation::run`` loads (reference
    src/linear_method/model_evaluation.h:16-27), on the host: whitespace
    separated ``key value`` pairs read as ``in >> k >> v``, a later pair
    overriding an earlier one within a file and across files (``weight[k] =
    v``).  Returns (sorted unique keys as uint64, their weights as float64).
    ``real=np.float32`` rounds each weight through ``float`` first, as the
    reference's ``Real`` does.  A trailing unpaired token, a key that is no
    uint64 and a value that is no number are errors.

    Defined deviation: after the last line of a file the reference's loop
    runs once more with a failed extraction and assigns ``weight[0]`` from it
    (model_evaluation.h:22-26: ``in.good()`` is still true after the last
    newline), so every loaded model there holds a key 0.  We do not add it."""
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    real = np.dtype(real)
    if real not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"real must be float64 or float32, not {real}")
    keys, vals = [], []
    for path in paths:
        with open(path, "r") as f:
            toks = f.read().split()
        if len(toks) % 2:
            raise ValueError(f"{path}: a key without a value ({toks[-1]!r})")
        for k in toks[0::2]:
            v = int(k) if k.isascii() and k.isdigit() else -1
            if not 0 <= v < (1 << 64):
                raise ValueError(f"{path}: {k!r} is no uint64 key")
            keys.append(v)
        try:
            vals.extend(float(v) for v in toks[1::2])
        except ValueError:
            raise ValueError(f"{path}: a value that is no number") from None
    k = np.array(keys, dtype=np.uint64)
    w = np.array(vals, dtype=np.float64).astype(real).astype(np.float64)
    # the last pair of each key: the first of the reversed list
    u, first = np.unique(k[::-1], return_index=True)
    return u, np.ascontiguousarray(w[::-1][first])


STATE_VERSION = 1
_STATE_ARRAYS = (("keys", np.uint64), ("pos", np.uint64), ("neg", np.uint64),
                 ("w", np.float64), ("z", np.float64))
_STATE_PARAMS = ("alpha", "beta", "lambda1", "lambda2")


def save_state(path, keys, pos, neg, w, z, alpha, beta, lambda1, lambda2, frozen=False,
               **extra) -> None:
    """One ``.npz`` at exactly ``path``: the five arrays of a model's image
    (``FTRLModel.state``), its four parameters as float64, ``frozen``, the
    format version, and the caller's ``extra`` arrays."""
    arrays = {name: np.ascontiguousarray(a, dtype=dt)
              for (name, dt), a in zip(_STATE_ARRAYS, (keys, pos, neg, w, z))}
    if len({a.size for a in arrays.values()}) != 1:
        raise ValueError("the five arrays of a model image have one length")
    for name, v in zip(_STATE_PARAMS, (alpha, beta, lambda1, lambda2)):
        arrays[name] = np.array(v, dtype=np.float64)
    arrays["frozen"] = np.array(1 if frozen else 0, dtype=np.int64)
    arrays["format_version"] = np.array(STATE_VERSION, dtype=np.int64)
    for name, v in extra.items():
        if name in arrays:
            raise ValueError(f"{name} is a field of the format")
        arrays[name] = np.asarray(v)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def load_state(path) -> dict:
    """The fields ``save_state`` wrote, by name; rejects any other version."""
    with np.load(path, allow_pickle=False) as f:
        if "format_version" not in f.files:
            raise ValueError(f"{path}: no FTRL model image (no format_version)")
        version = int(f["format_version"])
        if version != STATE_VERSION:
            raise ValueError(f"{path}: format version {version}, this reader knows "
                             f"{STATE_VERSION}")
        return {name: f[name] for name in f.files}


class FTRLModel:
    """FTRLModel<uint64, double> with its entries resident in HBM.

    The model is created on the device by the first call that needs it,
    with the learning rate and penalty set by then (the reference sets both
    in FTRL::init before any message arrives, ftrl.cc:10-17)."""

    def __init__(self, device: int = 0, capacity_hint: int = 0, flags: int = 0):
        self._L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._L.psg_create(device, PSG_F64, flags, C.byref(h)))
        self._h = h
        self._hint = capacity_hint
        self._alpha = self._beta = 1.0
        self._lambda1 = self._lambda2 = 0.0  # ftrl_model.h:49
        self._live = False

    def close(self):
        if getattr(self, "_h", None):
            self._L.psg_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- configuration: ftrl_model.h:15-22 ----------------------------------
    def setLearningRate(self, alpha: float, beta: float) -> None:
        self._need_fresh("setLearningRate")
        self._alpha, self._beta = float(alpha), float(beta)

    def setPenalty(self, lambda1: Optional[float] = None,
                   lambda2: Optional[float] = None) -> None:
        """PenaltyConfig.lambda(0) / lambda(1); None = not given (:20-21)."""
        self._need_fresh("setPenalty")
        if lambda1 is not None:
            self._lambda1 = float(lambda1)
        if lambda2 is not None:
            self._lambda2 = float(lambda2)

    def _need_fresh(self, what: str) -> None:
        if self._live:
            raise _lib.PSGError(_lib.PSG_ERR_ARG, what + " after the model's first message")

    def _model(self):
        if not self._live:
            p = _lib.FtrlParam(self._alpha, self._beta, self._lambda1, self._lambda2)
            _lib.check(self._L.psg_ftrl_init(self._h, C.byref(p), self._hint))
            self._live = True
        return self._h

    def reserve(self, entries: int) -> None:
        """Room for `entries` keys (psg_ftrl_reserve)."""
        _lib.check(self._L.psg_ftrl_reserve(self._model(), entries))

    # -- setValue: ftrl_model.h:80-112 ---------------------------------------
    def setValue(self, msg: Message) -> None:
        keys = np.ascontiguousarray(msg.key, dtype=np.uint64)
        if len(msg.value) != 3:  # CHECK_EQ(msg->value.size(), 3)
            raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{len(msg.value)} value arrays, FTRL needs 3")
        pos = np.ascontiguousarray(msg.value[0], dtype=np.uint32)
        neg = np.ascontiguousarray(msg.value[1], dtype=np.uint32)
        grad = np.ascontiguousarray(msg.value[2], dtype=np.float64)
        for a in (pos, neg, grad):  # CHECK_EQ(pos.size(), n) ... :86-88
            if a.size != keys.size:
                raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{a.size} values for {keys.size} keys")
        if keys.size == 0:
            return
        _lib.check(self._L.psg_ftrl_push(self._model(), _ptr(keys), keys.size, _ptr(pos),
                                         _ptr(neg), _ptr(grad)))

    # -- getValue: ftrl_model.h:72-78 ----------------------------------------
    def getValue(self, msg: Message) -> None:
        keys = np.ascontiguousarray(msg.key, dtype=np.uint64)
        out = np.zeros(keys.size, np.float64)
        if keys.size:
            _lib.check(self._L.psg_ftrl_pull(self._model(), _ptr(keys), keys.size, _ptr(out)))
        msg.value.append(out)

    # -- status: ftrl_model.h:31-32 ------------------------------------------
    def status(self):
        """(entries, nnz, norm1, norm2) of psg_ftrl_status."""
        e, z = C.c_size_t(), C.c_size_t()
        n1, n2 = C.c_double(), C.c_double()
        _lib.check(self._L.psg_ftrl_status(self._model(), C.byref(e), C.byref(z), C.byref(n1),
                                           C.byref(n2)))
        return e.value, z.value, n1.value, n2.value

    def objv(self) -> float:
        _, _, norm1, norm2 = self.status()
        return norm1 * self._lambda1 + .5 * self._lambda2 * math.sqrt(norm2)

    def nnz(self) -> int:
        return self.status()[1]

    def size(self) -> int:
        """Keys touched by a push (the reference's model_.size() also counts
        the keys a pull asked for)."""
        return self.status()[0]

    # -- dump: ftrl_model.h:24-29 --------------------------------------------
    def export(self):
        """(keys, w) of every nonzero weight, sorted by key."""
        n = C.c_size_t()
        rc = self._L.psg_ftrl_export(self._model(), None, None, 0, C.byref(n))
        if rc not in (_lib.PSG_OK, _lib.PSG_ERR_SIZE):
            _lib.check(rc)
        keys = np.empty(n.value, np.uint64)
        w = np.empty(n.value, np.float64)
        if n.value:
            _lib.check(self._L.psg_ftrl_export(self._h, _ptr(keys), _ptr(w), n.value,
                                               C.byref(n)))
        order = np.argsort(keys, kind="stable")
        return keys[order], w[order]

    def lookup(self, keys):
        """Whole entries (psg_ftrl_lookup): pos, neg, w, z, found."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        pos, neg = np.zeros(k.size, np.uint64), np.zeros(k.size, np.uint64)
        w, z = np.zeros(k.size, np.float64), np.zeros(k.size, np.float64)
        found = np.zeros(k.size, np.uint8)
        if k.size:
            _lib.check(self._L.psg_ftrl_lookup(self._model(), _ptr(k), k.size, _ptr(pos),
                                               _ptr(neg), _ptr(w), _ptr(z), _ptr(found)))
        return pos, neg, w, z, found

    # -- checkpoint: the hooks ftrl_model.h:41-44 leaves empty ----------------
    def state(self, range=None):
        """getReplica: (keys, pos, neg, w, z) of every entry whose key lies in
        the closed interval ``range = (first, last)`` (None: all), sorted by
        key on the device (psg_ftrl_export_state)."""
        r = None
        if range is not None:
            r = (C.c_uint64 * 2)(int(range[0]), int(range[1]))
        n = C.c_size_t()
        rc = self._L.psg_ftrl_export_state(self._model(), r, None, None, None, None, None, 0,
                                           C.byref(n))
        if rc not in (_lib.PSG_OK, _lib.PSG_ERR_SIZE):
            _lib.check(rc)
        out = [np.empty(n.value, dt) for _, dt in _STATE_ARRAYS]
        if n.value:
            _lib.check(self._L.psg_ftrl_export_state(self._h, r, *[_ptr(a) for a in out],
                                                     n.value, C.byref(n)))
        return tuple(out)

    def restore(self, keys, pos=None, neg=None, w=None, z=None) -> None:
        """recoverFrom / setReplica: an upsert of whole entries, strictly
        increasing by key (psg_ftrl_import).  ``pos``, ``neg`` and ``z`` all
        None: the weights-only form, which freezes the model."""
        if w is None:
            raise _lib.PSGError(_lib.PSG_ERR_ARG, "restore needs the weights")
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        rest = [None if a is None else np.ascontiguousarray(a, dtype=dt)
                for a, dt in ((pos, np.uint64), (neg, np.uint64), (z, np.float64))]
        for a in [w] + [a for a in rest if a is not None]:
            if a.size != keys.size:
                raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{a.size} values for {keys.size} keys")
        p = [None if a is None else _ptr(a) for a in rest]
        _lib.check(self._L.psg_ftrl_import(self._model(), _ptr(keys), keys.size, p[0], p[1],
                                           _ptr(w), p[2]))

    @property
    def frozen(self) -> bool:
        """Evaluation only: loaded by a weights-only import (psg_ftrl_frozen)."""
        f = C.c_int()
        _lib.check(self._L.psg_ftrl_frozen(self._model(), C.byref(f)))
        return bool(f.value)

    def save(self, path, **extra) -> None:
        """The model's image, parameters and ``extra`` arrays in one ``.npz``
        (``save_state``)."""
        frozen = self.frozen
        save_state(path, *self.state(), self._alpha, self._beta, self._lambda1, self._lambda2,
                   frozen=frozen, **extra)

    @classmethod
    def from_state(cls, st: dict, device: int = 0, flags: int = 0) -> "FTRLModel":
        """A model holding what ``load_state`` read.  The parameters come back
        by bits; a frozen model comes back through the weights-only import,
        frozen."""
        m = cls(device, capacity_hint=int(st["keys"].size), flags=flags)
        m._alpha, m._beta, m._lambda1, m._lambda2 = (float(st[k]) for k in _STATE_PARAMS)
        if int(st["frozen"]):
            m.restore(st["keys"], w=st["w"])
        else:
            m.restore(st["keys"], st["pos"], st["neg"], st["w"], st["z"])
        m._model()
        return m

    @classmethod
    def load(cls, path, device: int = 0) -> "FTRLModel":
        return cls.from_state(load_state(path), device)

    def readFromFile(self, paths, real=np.float64) -> None:
        """The first half of ModelEvaluation::run (model_evaluation.h:16-27):
        ``read_model_text`` of the files, then the weights-only import.  The
        model is evaluation-only afterwards: pulls work, pushes are refused."""
        keys, w = read_model_text(paths, real)
        self.restore(keys, w=w)

    def writeToFile(self, path: str) -> None:
        """One ``key\\tw`` line per nonzero weight, sorted by key (the
        reference writes them in its hash map's order, which is unspecified)."""
        keys, w = self.export()
        with open(path, "w") as f:
            for k, v in zip(keys.tolist(), w.tolist()):
                f.write("%d\t%s\n" % (k, format_weight(v)))
