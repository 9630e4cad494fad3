"""Python mirror of the reference's online server model over the C ABI.

``FTRLModel`` follows ``PS::LM::FTRLModel<Key, double>`` (reference
src/linear_method/ftrl_model.h:12-69) method for method --
``setLearningRate``, ``setPenalty``, ``setValue``, ``getValue``, ``objv``,
``nnz``, ``writeToFile`` -- over the hash table resident in HBM behind
``psg_ftrl_*`` (include/psg.h, which also lists the defined deviations: a
pull does not insert, the norms are a reduction, a message must be strictly
increasing, the dump is sorted by key).
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

    def writeToFile(self, path: str) -> None:
        """One ``key\\tw`` line per nonzero weight, sorted by key (the
        reference writes them in its hash map's order, which is unspecified)."""
        keys, w = self.export()
        with open(path, "w") as f:
            for k, v in zip(keys.tolist(), w.tolist()):
                f.write("%d\t%s\n" % (k, format_weight(v)))
