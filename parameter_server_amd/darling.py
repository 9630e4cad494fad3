"""Python mirror of the worker half of the batch solver over the C ABI.

``DarlingWorker`` is a thin class over ``psg_mb_darling_*`` (include/psg.h):
the worker's data of one feature group resident in HBM as a localized
``Minibatch``, with ``Darling::computeGradients`` (reference
src/linear_method/darling.cc:306-356), ``updateDual`` (:358-435), the
worker's lines of ``preprocessData`` (:110-117) and ``evaluateProgress``
(:506) as device kernels.  The dictionary is ``w_->key(grp)`` and the
dictionary positions ``[cb, ce)`` are the reference's ``seg_pos``.

``block_step`` is one worker pass of ``Darling::updateModel`` (:203-250)
against a ``KVVector`` server in the same context with G, U and the pulled
weights passing through the host (``psg_push``, ``psg_darling_update``,
``psg_gather``): five host waits per block.  It is kept as the comparison
path of the device form.

``push_block`` / ``pull_block`` / ``block_step_dev`` are the same pass over
the context's device-array forms (``psg_push_dev``, ``psg_darling_update_dev``,
``psg_pull_dev``): G and U go from ``psg_mb_darling_gradients``' scratch block
into the server's aggregate and the pulled weights from the server's values
into ``psg_mb_darling_update_dual`` without leaving HBM, all enqueued on the
minibatch's stream, with no host wait.  ``darling_pass`` drives a whole pass
over the key blocks for W workers that way, and ``server_progress`` is the
server branch of ``evaluateProgress`` (:538-555), the one place that waits.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

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
    _GU = 0           # scratch slot of the minibatch: (G, U) of a block
    _PULL = 1         # ... and the block's pulled weights (device forms)

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

    def load_group(self, reader, slot_id: int, dict_keys, w=None, dual_of=None) -> None:
        """``load`` for feature group ``slot_id`` of ``reader`` (a
        ``slots.SlotReader`` on this worker's context) with no host copy of
        the matrix: psg_mb_group_extract, uniq, localize, psg_mb_darling_init.
        ``dual_of``: another DarlingWorker (already loaded, over the same
        rows) whose dual this one shares (psg_mb_darling_share_dual), as the
        groups of a reference worker share dual_; ``w`` must then be None, and
        every call on the sharing workers has to be given one stream (the
        default does: they are on one context)."""
        dict_keys = np.ascontiguousarray(dict_keys, dtype=np.uint64)
        if dual_of is not None and w is not None:
            raise _lib.PSGError(_lib.PSG_ERR_ARG, "weights for a worker that shares a dual")
        mb = self.mb
        reader.extract(slot_id, mb)
        mb.uniq()
        mb.localize(self._upload(self._DICT, dict_keys), dict_keys.size)
        w_dev = None
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float64)
            if w.size != dict_keys.size:
                raise _lib.PSGError(_lib.PSG_ERR_SIZE, f"{w.size} weights, {dict_keys.size} keys")
            w_dev = self._upload(self._W, w)
        if dual_of is not None:
            _lib.check(self._L.psg_mb_darling_share_dual(mb._h, dual_of.mb._h))
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

    # ---- the same pass with G, U and the weights resident (device forms) ----
    def reserve_block(self, ncols: int) -> None:
        """Scratch for blocks of up to ``ncols`` columns.  A scratch block
        that grows is reallocated, which waits for the device: sized once for
        the widest block, no later push_block / pull_block allocates."""
        self.mb.scratch(self._GU, max(16 * ncols, 8))
        self.mb.scratch(self._PULL, max(8 * ncols, 8))

    def _key_range(self, cb: int, ce: int) -> tuple:
        return (int(self.dict_keys[cb]),
                int(self.dict_keys[ce]) if ce < self.ndict else (1 << 64) - 1)

    def push_block(self, server: KVVector, chl: int, time: int, cb: int, ce: int,
                   key_range: Optional[tuple] = None, slice: Optional[int] = None) -> None:
        """computeGradients over columns [cb, ce) (:208) and the push of
        (G, U) as one m = 2 message at ``time`` (:215-220), enqueued on the
        minibatch's stream: psg_mb_darling_gradients into scratch, then
        psg_push_dev of the dictionary's device slice with the two arrays.
        ``slice``: the claim that these keys are the server's
        key(chl)[slice, slice + ce - cb) (psg_push_dev).  No host wait; a
        no-op for ce <= cb (seg_pos.empty())."""
        if ce <= cb:
            return
        m = ce - cb
        if key_range is None:
            key_range = self._key_range(cb, ce)
        s = self.mb.stream
        p = self.mb.scratch(self._GU, 16 * m)
        _lib.check(self._L.psg_mb_darling_gradients(self.mb._h, cb, ce, p, p + 8 * m, s))
        server.push_dev(chl, time, key_range, self._dev[self._DICT].data_ptr() + 8 * cb, m,
                        [p, p + 8 * m], slice=slice, stream=s)

    def pull_block(self, server: KVVector, chl: int, cb: int, ce: int) -> None:
        """The pull of the block's weights (:225-250) into scratch by
        psg_pull_dev, then updateDual from them (:238).  No host wait; a no-op
        for ce <= cb."""
        if ce <= cb:
            return
        m = ce - cb
        s = self.mb.stream
        p = self.mb.scratch(self._PULL, 8 * m)
        server.pull_dev(chl, self._dev[self._DICT].data_ptr() + 8 * cb, m, p, stream=s)
        _lib.check(self._L.psg_mb_darling_update_dual(self.mb._h, cb, ce, p, self.delta_max, s))

    def block_step_dev(self, server: KVVector, chl: int, time: int, cb: int, ce: int,
                       param: dict, key_range: Optional[tuple] = None,
                       slice: Optional[int] = None) -> None:
        """block_step for a single worker with nothing crossing the host:
        push_block, psg_darling_update_dev, pull_block.  The block's violation
        is accumulated on the server (server_progress reads it)."""
        if ce <= cb:
            return
        self.push_block(server, chl, time, cb, ce, key_range, slice)
        server_update_dev(server, chl, time, param, self.delta_max)
        self.pull_block(server, chl, cb, ce)


def server_update_dev(server: KVVector, chl: int, time: int, param: dict,
                      delta_max: float) -> None:
    """The server's UPDATE_MODEL step on the aggregate of ``time``
    (psg_darling_update_dev): enqueued, no host wait."""
    p = _lib.DarlingParam(param["eta"], param["lambda_"], param["kkt_filter_threshold"],
                          delta_max)
    _lib.check(server._L.psg_darling_update_dev(server._h, chl, time,
                                                C.cast(C.byref(p), C.c_void_p)))


def block_columns(dict_keys: np.ndarray, kb: int, ke: int) -> Tuple[int, int]:
    """A worker's columns [cb, ce) of the global key block [kb, ke): the
    positions of its dictionary's keys in the block, SArray::findRange's two
    lower_bounds (psg_find_range's rule).  Pure numpy."""
    d = np.asarray(dict_keys, dtype=np.uint64)
    cb = int(np.searchsorted(d, np.uint64(kb), side="left"))
    ce = int(np.searchsorted(d, np.uint64(ke), side="left"))
    return cb, max(ce, cb)


def pass_schedule(dicts: Sequence[np.ndarray], key_blocks: Sequence[tuple]) -> List[list]:
    """For every key block of ``key_blocks``, in order, the (worker, cb, ce) of
    each worker that holds a key of it (ce > cb); an empty list where none
    does.  Pure numpy: darling_pass's block-to-columns mapping."""
    out = []
    for kb, ke in key_blocks:
        row = []
        for w, d in enumerate(dicts):
            cb, ce = block_columns(d, kb, ke)
            if ce > cb:
                row.append((w, cb, ce))
        out.append(row)
    return out


def darling_pass(server: KVVector, workers: Sequence[DarlingWorker], chl: int, time: int,
                 key_blocks: Sequence[tuple], param: dict) -> int:
    """One data pass of Darling::updateModel (:196-267) for W workers against
    ``server``, with no host wait inside the pass.  For each global key block
    [kb, ke) of ``key_blocks``, in the given order: every worker holding a
    key of it pushes (push_block, key_range = the block), the server updates
    once (psg_darling_update_dev), then every such worker pulls (pull_block).
    Blocks run strictly one after another -- max_block_delay = 0; the
    reference's bounded-delay schedule (darling.cc:44-58) is not built.  Time
    advances by 3 per block (the push at t, the server's update at t + 1 and
    the pull at t + 2 of :215-250 are one block's times); a block in which no
    worker holds a key is skipped, time included: nothing is pushed, so there
    is no aggregate to update (the reference would CHECK-fail in received).
    Returns the time after the last block.  Errors found on the device are
    reported by server.dev_status() or server_progress()."""
    sched = pass_schedule([w.dict_keys for w in workers], key_blocks)
    for w in workers:
        w.reserve_block(max([ce - cb for row in sched for i, cb, ce in row
                             if workers[i] is w], default=0))
    delta_max = workers[0].delta_max if workers else 0.0
    for (kb, ke), row in zip(key_blocks, sched):
        if not row:
            continue
        for i, cb, ce in row:
            workers[i].push_block(server, chl, time, cb, ce, key_range=(int(kb), int(ke)))
        server_update_dev(server, chl, time, param, delta_max)
        for i, cb, ce in row:
            workers[i].pull_block(server, chl, cb, ce)
        time += 3
    return time


def server_progress(server: KVVector, chl: int, lambda_: float,
                    reset_violation: bool = False) -> dict:
    """The server branch of evaluateProgress (:538-555) by
    psg_darling_progress: nnz_w, objv = lambda * sum |w|, the violation
    accumulated since the last reset, nnz_active.  Waits for the device and
    raises the deferred error of the device forms, if any."""
    nnz_w, nnz_as = C.c_size_t(), C.c_size_t()
    objv, vio = C.c_double(), C.c_double()
    _lib.check(server._L.psg_darling_progress(server._h, chl, float(lambda_),
                                              1 if reset_violation else 0, C.byref(nnz_w),
                                              C.byref(objv), C.byref(vio), C.byref(nnz_as)))
    return {"nnz_w": nnz_w.value, "objv": objv.value, "violation": vio.value,
            "nnz_active": nnz_as.value}
