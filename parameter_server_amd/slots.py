"""Text ingest by feature group over the C ABI: the batch solver's data path.

``SlotReader`` mirrors the reference's ``SlotReader::read``
(src/data/slot_reader.cc:35-232): ADFEA / LIBSVM text parsed with
``ignore_feature_group = false``, the ``ExampleInfo`` of the load
(``ExampleParser::toProto`` / ``info``, src/data/example_parser.cc:38-82) and
one matrix per slot id, here one resident ``Minibatch`` per group
(``psg_mb_groups`` / ``psg_mb_group_extract``, include/psg.h).  The text is
parsed on the device (``psg_mb_load_text_groups``); the grouping, the
statistics and the extraction run there too, so no matrix crosses the host.
``parse_text_groups_host`` / ``parse_groups_skipping`` are the same parse done
serially on the host, for callers without a device.

``merge_example_info`` is ``mergeExampleInfo`` (src/data/common.cc:46-69) and
``feature_blocks`` the partition of ``BatchSolver::run``
(src/linear_method/batch_solver.cc:48-66).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Tuple

import numpy as np

from . import _lib
from .kv_vector import _ptr
from .worker import Minibatch, _format

SLOT_MAX = 4096  # kSlotIDmax: the ids are 1 .. 4095


def parse_text_groups_host(text: bytes, fmt, max_rows=None, final: bool = True):
    """psg_text_parse_groups_host: (offset, index, value or None, y, slot,
    result), parsed serially on the host."""
    L = _lib.lib()
    text = bytes(text)
    f = _format(fmt)
    cap = (1 << 64) - 1 if max_rows is None else int(max_rows)
    r = _lib.TextResult()
    _lib.check(L.psg_text_parse_groups_host(text, len(text), f, cap, 1 if final else 0, None, None,
                                            None, None, None, 0, 0, C.byref(r)))
    offset = np.zeros(r.rows + 1, np.uint64)
    index = np.zeros(r.nnz, np.uint64)
    value = np.zeros(r.nnz, np.float64) if f == _lib.PSG_TEXT_LIBSVM else None
    y = np.zeros(r.rows, np.float64)
    slot = np.zeros(r.nnz, np.uint16)
    _lib.check(L.psg_text_parse_groups_host(
        text, len(text), f, cap, 1 if final else 0, _ptr(offset), _ptr(index),
        _ptr(value) if value is not None else None, _ptr(y), _ptr(slot), int(r.rows), int(r.nnz),
        C.byref(r)))
    return offset, index, value, y, slot, r


def _lines(text: bytes, final: bool) -> List[bytes]:
    """The lines of the grouped parse, each with its '\\n'; a last line
    without one counts when ``final``."""
    out, at = [], 0
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            break
        out.append(text[at:nl + 1])
        at = nl + 1
    if final and at < len(text):
        out.append(text[at:])
    return out


class _Kept:
    """The lines still in the buffer and their numbers in the text given."""

    def __init__(self, text: bytes, final: bool):
        self.lines = _lines(bytes(text), final)
        self.orig = list(range(len(self.lines)))
        self.bad: List[int] = []

    def text(self) -> bytes:
        return b"".join(self.lines)

    def drop(self, i: int) -> None:
        self.bad.append(self.orig[i])
        del self.lines[i], self.orig[i]


def _parse_kept(kept: _Kept, fmt, skip_bad: bool):
    while True:
        # every kept line ends in '\n' or is the last: the buffer is final
        offset, index, value, y, slot, r = parse_text_groups_host(kept.text(), fmt, None, True)
        if r.bad_line < 0:
            return offset, index, value, y, slot
        if not skip_bad:
            raise _lib.PSGError(_lib.PSG_ERR_ARG,
                                f"line {kept.orig[r.bad_line]} of the text is rejected")
        kept.drop(int(r.bad_line))


def parse_groups_skipping(text: bytes, fmt, skip_bad: bool = True, final: bool = True):
    """The grouped host parse of all of ``text`` with SlotReader's skip
    (slot_reader.cc:148): a line the parse rejects is cut out of the buffer
    and the buffer is parsed again, so a skipped line has no effect.  Returns
    (offset, index, value or None, y, slot, bad_lines); ``bad_lines`` are the
    skipped lines' numbers in ``text``.  Without ``skip_bad`` a rejected line
    raises PSGError(PSG_ERR_ARG)."""
    kept = _Kept(text, final)
    return _parse_kept(kept, fmt, skip_bad) + (list(kept.bad),)


def info_dict(s: "_lib.SlotInfo") -> dict:
    return {"id": int(s.id), "format": int(s.format), "min_key": int(s.min_key),
            "max_key": int(s.max_key), "nnz_ele": int(s.nnz_ele), "nnz_ex": int(s.nnz_ex)}


def mb_groups(mb: Minibatch) -> Tuple[List[dict], int]:
    """psg_mb_groups: (the slots' info in ascending id order, bad_row).  With
    bad_row >= 0 the list is empty."""
    L = _lib.lib()
    buf = (_lib.SlotInfo * SLOT_MAX)()
    n, bad = C.c_size_t(), C.c_int64(-1)
    rc = L.psg_mb_groups(mb._h, buf, SLOT_MAX, C.byref(n), C.byref(bad))
    if rc == _lib.PSG_ERR_ARG and bad.value >= 0:
        return [], int(bad.value)
    _lib.check(rc)
    return [info_dict(buf[i]) for i in range(n.value)], -1


def mb_set_slots(mb: Minibatch, slot) -> None:
    """psg_mb_set_slots: one uint16 slot id per entry of the loaded minibatch."""
    slot = np.ascontiguousarray(slot, dtype=np.uint16)
    _lib.check(_lib.lib().psg_mb_set_slots(mb._h, _ptr(slot) if slot.size else None, slot.size))


def mb_group_extract(src: Minibatch, slot_id: int, dst: Minibatch, nnz: int = 0) -> None:
    """psg_mb_group_extract; ``nnz``: the group's entries (its info's nnz_ele)."""
    _lib.check(_lib.lib().psg_mb_group_extract(src._h, int(slot_id), dst._h))
    dst.rows, dst.nnz = src.rows, int(nnz)
    dst.n_uniq = dst.ndict = 0


class SlotReader:
    """One load of grouped text, resident on the device of context ``ctx`` (a
    ``psg_ctx`` handle of a PSG_F64 context)."""

    def __init__(self, ctx):
        self.mb = Minibatch(ctx)
        self.info: List[dict] = []
        self.num_ex = 0
        self.bad_lines: List[int] = []

    def close(self):
        self.mb.close()

    def read(self, text: bytes, fmt, skip_bad: bool = True, final: bool = True) -> List[dict]:
        """The grouped load of ``text`` ("adfea", "libsvm" or a PSG_TEXT_* id)
        and psg_mb_groups.  With ``skip_bad`` a line that either stage
        reports (the parse: a rejected line; the grouping: a slot id in two
        separate runs of a row) is cut out of the host buffer and the buffer
        is read again, so a skipped line has no effect; the skipped lines'
        numbers are kept in ``bad_lines``.  Without it such a line raises.
        Returns ``info``: one dict per slot (id, format, min_key, max_key,
        nnz_ele, nnz_ex) in ascending id order, the label slot 0 first;
        ``num_ex`` is the examples loaded."""
        kept = _Kept(text, final)
        while True:
            # every kept line ends in '\n' or is the last: the buffer is final
            r = self.mb.load_text_groups(kept.text(), fmt, None, True)
            bad, why = int(r.bad_line), "is rejected"
            if bad < 0:
                info, bad = mb_groups(self.mb)  # every kept line is a row: row r is kept line r
                why = "holds a slot id in two separate runs"
                if bad < 0:
                    break
            if not skip_bad:
                raise _lib.PSGError(_lib.PSG_ERR_ARG, f"line {kept.orig[bad]} of the text {why}")
            kept.drop(bad)
        self.info, self.num_ex = info, int(r.rows)
        self.bad_lines = sorted(kept.bad)
        return info

    def example_info(self) -> dict:
        """The load's ExampleInfo: {"num_ex", "slot": info}."""
        return {"num_ex": self.num_ex, "slot": list(self.info)}

    def slots(self) -> List[int]:
        """The feature slots present (the label slot 0 left out)."""
        return [s["id"] for s in self.info if s["id"] != 0]

    def extract(self, slot_id: int, minibatch: Minibatch) -> None:
        """SlotReader::index / offset / value of one slot as ``minibatch``
        (of the same context): num_ex rows, the group's entries in their
        original order; an absent slot gives empty rows."""
        nnz = next((s["nnz_ele"] for s in self.info if s["id"] == slot_id), 0)
        mb_group_extract(self.mb, slot_id, minibatch, nnz)


def merge_example_info(a: dict, b: dict) -> dict:
    """mergeExampleInfo (data/common.cc:46-69) of two ExampleInfo dicts
    ({"num_ex", "slot": [slot dicts]}): slots by id, min / max of the key
    range, sums of nnz_ele and nnz_ex; two formats for one id raise (the
    reference's CHECK_EQ)."""
    slots = {s["id"]: dict(s) for s in a["slot"]}
    for s in b["slot"]:
        t = slots.get(s["id"])
        if t is None:
            slots[s["id"]] = dict(s)
            continue
        if t["format"] != s["format"]:
            raise ValueError("slot %d: formats %d and %d" % (s["id"], t["format"], s["format"]))
        t["min_key"] = min(t["min_key"], s["min_key"])
        t["max_key"] = max(t["max_key"], s["max_key"])
        t["nnz_ele"] += s["nnz_ele"]
        t["nnz_ex"] += s["nnz_ex"]
    return {"num_ex": a["num_ex"] + b["num_ex"], "slot": [slots[i] for i in sorted(slots)]}


def even_divide(begin: int, end: int, n: int) -> np.ndarray:
    """psg_even_divide: the n + 1 bounds of Range(begin, end).evenDivide(n, i)."""
    out = np.zeros(n + 1, np.uint64)
    _lib.check(_lib.lib().psg_even_divide(int(begin), int(end), n,
                                          out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def feature_blocks(info, feature_block_ratio: float) -> List[Tuple[int, int, int]]:
    """The feature blocks of batch_solver.cc:48-66 as (grp, kb, ke): each
    feature slot's [min_key, max_key) cut evenly into n blocks, n = 1 unless
    nnz_ele / nnz_ex > 1 + 1e-6, then max(ceil(nnz_per_row * ratio), 1);
    empty blocks are dropped and the label slot is skipped.  ``info``: an
    ExampleInfo dict or its slot list."""
    slots = info["slot"] if isinstance(info, dict) else info
    out = []
    for s in slots:
        if s["id"] == 0:
            continue
        nnz_per_row = float(s["nnz_ele"]) / float(s["nnz_ex"])
        n = 1
        if nnz_per_row > 1 + 1e-6:
            n = max(int(math.ceil(nnz_per_row * float(feature_block_ratio))), 1)
        b = even_divide(s["min_key"], s["max_key"], n)
        for i in range(n):
            kb, ke = int(b[i]), int(b[i + 1])
            if kb >= ke:  # Range::empty()
                continue
            out.append((s["id"], kb, ke))
    return out
