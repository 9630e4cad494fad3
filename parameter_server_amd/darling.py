"""Python mirror of the worker half of the batch solver over the C ABI.

``DarlingWorker`` is a thin class over ``psg_mb_darling_*`` (include/psg.h):
the worker's data of one feature group resident in HBM as a localized
``Minibatch``, with ``Darling::computeGradients`` (reference
src/linear_method/darling.cc:306-356), ``updateDual`` (:358-435), the
worker's lines of ``preprocessData`` (:110-117) and ``evaluateProgress``
(:506) as device kernels.  The dictionary is ``w_->key(grp)`` and the
dictionary positions ``[cb, ce)`` are the reference's ``seg_pos``.

``block_step`` is one worker pass of ``Darling::updateModel`` (:203-250)
against a ``KVVector`` server in the same context.  G, U and the pulled
weights pass through the host there: the KVVector push (``psg_push``) and
gather (``psg_gather``) take host arrays and have no device-pointer forms.
Adding those is a separate change; the kernels on both sides already read and
write device arrays.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .kv_vector import KVVector, Message, _ptr
from .worker import Minibatch

# psg_mb_read's arrays of the Darling state: name -> (id, dtype)
STATE = {
    "dual": (_lib.PSG_MB_DARLING_DUAL, np.float64),
    "cur_w": (_lib.PSG_MB_DARLING_CUR_W, np.float64),
    "delta": (_lib.PSG_MB_DARLING_DELTA, np.float64),
    "active": (_lib.PSG_MB_DARLING_ACTIVE, np.uint8),
    "delta_w": (_lib.PSG_MB_DARLING_DELTA_W, np.float64),
}


class DarlingWorker:
    """The worker of the batch solver (darling.cc:196-250) for one feature
    group on the device of context ``ctx`` (a ``psg_ctx`` handle of a PSG_F64
    context, e.g. ``KVVector(0, PSG_F64)._h``).  ``delta_init`` and
    ``delta_max`` are conf_.darling()'s delta_init_value and delta_max_value."""

    _DICT, _W = 0, 1  # uploaded blocks
    _GU = 0           # scratch slot of the minibatch

    def __init__(self, ctx, delta_init: float, delta_max: float, device: int = 0):
        self._L = _lib.lib()
        self._ctx = ctx
        self.device = device
        self.delta_init = float(delta_init)
        self.delta_max = float(delta_max)
        self.mb = Minibatch(ctx)
        self._dev = {}
        self.dict_keys = np.zeros(0, np.uint64)
        self.ndict = 0

    def close(self):
        self.mb.close()  # waits for the minibatch's work
        self._dev = {}

    def _upload(self, slot: int, a: np.ndarray) -> int:
        """A host array as a device block that lives until the next upload to
        `slot`.  The device-wide wait covers the copy and whatever kernel
        still reads the block this one replaces."""
        import torch
        dev = "cuda:%d" % self.device
        if a.nbytes:
            t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)
        else:
            t = torch.zeros(8, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(self.device)
        self._dev[slot] = t
        return t.data_ptr()

    def load(self, offset, index, value, y, dict_keys, w=None) -> None:
        """The worker's data (row-major CSR with global ids, ``value`` None: a
        binary matrix), its dictionary (strictly increasing) and,
        optionally, the weights it starts from (preprocessData, :106-117)."""
        dict_keys = np.ascontiguousarray(dict_keys, dtype=np.uint64)
        mb = self.mb
        mb.load(offset, index, value, y)
        mb.uniq()
        mb.localize(self._upload(self._DICT, dict_keys), dict_keys.size)
        w_dev = None
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float64)
            if w.size != dict_keys.size:
                raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{w.size} weights, {dict_keys.size} keys")
            w_dev = self._upload(self._W, w)
        _lib.check(self._L.psg_mb_darling_init(mb._h, self.delta_init, w_dev, None))
        self.dict_keys, self.ndict = dict_keys, dict_keys.size

    def reset_active(self) -> None:
        """kkt_filter_reset (:167-169)."""
        _lib.check(self._L.psg_mb_darling_reset_active(self.mb._h, None))

    def gradients(self, cb: int, ce: int) -> Tuple[np.ndarray, np.ndarray]:
        """computeGradients over columns [cb, ce): host copies of (G, U)."""
        m = max(ce - cb, 0)
        p = self.mb.scratch(self._GU, max(16 * m, 8))
        _lib.check(self._L.psg_mb_darling_gradients(self.mb._h, cb, ce, p, p + 8 * m, None))
        gu = self.mb.read_scratch(self._GU, np.float64, 2 * m)
        return gu[:m].copy(), gu[m:].copy()

    def update_dual(self, cb: int, ce: int, new_w) -> None:
        """updateDual with the pulled weights of columns [cb, ce)."""
        new_w = np.ascontiguousarray(new_w, dtype=np.float64)
        if new_w.size != max(ce - cb, 0):
            raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{new_w.size} weights for [{cb}, {ce})")
        p = self._upload(self._W, new_w)
        _lib.check(self._L.psg_mb_darling_update_dual(self.mb._h, cb, ce, p, self.delta_max,
                                                      None))

    def objv(self) -> float:
        """evaluateProgress (:506): sum log(1 + 1 / dual)."""
        v = C.c_double()
        _lib.check(self._L.psg_mb_darling_objv(self.mb._h, C.byref(v), None))
        return v.value

    def state(self) -> dict:
        """Host copies of dual, cur_w, delta, active (bytes) and the last delta_w."""
        return {name: self.mb._read(what, dtype) for name, (what, dtype) in STATE.items()}

    def set_state(self, dual=None, cur_w=None, delta=None, active=None) -> None:
        def arr(a, dtype, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.size != n:
                raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{a.size} items, {n} expected")
            return a
        a = [arr(dual, np.float64, self.mb.rows), arr(cur_w, np.float64, self.ndict),
             arr(delta, np.float64, self.ndict), arr(active, np.uint8, self.ndict)]
        _lib.check(self._L.psg_mb_darling_set_state(
            self.mb._h, *[_ptr(x) if x is not None and x.size else None for x in a]))

    def block_step(self, server: KVVector, chl: int, time: int, cb: int, ce: int,
                   param: dict, key_range: Optional[tuple] = None) -> float:
        """One worker pass of darling.cc:203-250 over columns [cb, ce) against
        ``server`` (a PSG_F64 KVVector on this worker's context whose
        key(chl) holds the dictionary and on which psg_darling_init has run):
        push (G, U) as one m = 2 message at ``time``, the server's
        updateWeight (psg_darling_update) with ``param`` = {eta, lambda_,
        kkt_filter_threshold}, pull the block's weights, updateDual.  Returns
        the block's violation.  G, U and the weights cross the host: see the
        module docstring."""
        if ce <= cb:  # seg_pos.empty(): nothing is pushed or pulled
            return 0.0
        keys = self.dict_keys[cb:ce]
        if key_range is None:
            key_range = (int(keys[0]),
                         int(self.dict_keys[ce]) if ce < self.ndict else (1 << 64) - 1)
        G, U = self.gradients(cb, ce)                                      # :208
        server.setValue(Message(time=time, key_channel=chl, key_range=key_range, key=keys,
                                value=[G, U]))                             # :215-220
        p = _lib.DarlingParam(param["eta"], param["lambda_"], param["kkt_filter_threshold"],
                              self.delta_max)
        vio = C.c_double()
        _lib.check(self._L.psg_darling_update(server._h, chl, time, C.cast(C.byref(p), C.c_void_p),
                                              C.byref(vio)))               # :259-267
        pull = Message(key_channel=chl, key=keys)
        server.getValue(pull)                                              # :225-250
        self.update_dual(cb, ce, pull.value[0])                            # :238
        return vio.value
