"""SlotReader's cache files, written and loaded on the device.

``CachedSlotReader`` is the reference's ``SlotReader`` over a list of text
files (src/data/slot_reader.cc:35-290): every file is parsed in chunks of
bounded size, each chunk's slots are appended to the per-(file, slot) cache
files ``.colidx`` (uint64), ``.rowsiz`` (uint16) and ``.value`` (float), each
a sequence of snappy streams listed as ``start\\tsize`` lines in a
``.partition`` file, and the file's ``ExampleInfo`` is kept as ``.info`` in
protobuf text format.  A file whose ``.info`` exists is not parsed again
(``hit_cache``).  ``extract`` rebuilds one slot of all the files as one
resident minibatch (``psg_mb_load_cache``): the streams are decoded on the
device, the row sizes scanned into offsets there.

The arrays are made by ``psg_mb_cache_pack`` from the chunk's extracted group;
only the zero padding of a slot that skips rows (slot_reader.cc:158-161,
215-218) and the label slot's all-ones row sizes are made on the host, with
the compressor's host twin.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .kv_vector import _ptr
from .slots import SlotReader, merge_example_info
from .snappy import compress_host
from .worker import Minibatch, _format

MIN_CHUNK_BYTES = 128 << 10  # a line of 61439 bytes or more is rejected by the parse anyway
DEFAULT_CHUNK_BYTES = 32 << 20
# Raw bytes per partition.  The decode runs one workgroup per partition, so the
# partitions of a load are its parallelism: of 4 KiB .. 1 MiB measured
# (profiles/slot_cache.json) 16 KiB loads within a third of the
# fastest (4 KiB) with a tenth fewer bytes, and six times faster than 64 KiB.
DEFAULT_PART_BYTES = 16 << 10

FORMAT_NAMES = {_lib.PSG_SLOT_DENSE: "DENSE", _lib.PSG_SLOT_SPARSE: "SPARSE",
                _lib.PSG_SLOT_SPARSE_BINARY: "SPARSE_BINARY"}
_FORMAT_IDS = {v: k for k, v in FORMAT_NAMES.items()}
_EXT = {_lib.PSG_CACHE_COLIDX: ".colidx", _lib.PSG_CACHE_ROWSIZ: ".rowsiz",
        _lib.PSG_CACHE_VALUE: ".value"}


# ---- names ------------------------------------------------------------------
def djb_hash32(s) -> int:
    """DJBHash32 (util/common.h:103-109) of the path as given.  The reference
    iterates ``const char&``: a byte >= 0x80 is sign-extended before the add."""
    b = s.encode() if isinstance(s, str) else bytes(s)
    h = 5381
    for c in b:
        h = (h * 33 + (c if c < 0x80 else c + 0xFFFFFF00)) & 0xFFFFFFFF
    return h


def _filename(path: str) -> str:
    """getFilename (util/file.cc:303-306): the last item of a getline split at '/'."""
    items = path.split("/")
    if items and items[-1] == "":
        items.pop()  # getline yields nothing after a trailing delimiter
    return items[-1] if items else ""


def _stem(prefix: str, path: str) -> str:
    return prefix + str(djb_hash32(path)) + "-" + _filename(path)


def cache_name(prefix: str, path: str, slot_id: int) -> str:
    """SlotReader::cacheName (slot_reader.cc:21-25); ``prefix`` is concatenated as given."""
    return _stem(prefix, path) + "_slot_" + str(int(slot_id))


def info_name(prefix: str, path: str) -> str:
    """The file's ExampleInfo (slot_reader.cc:70-71)."""
    return _stem(prefix, path) + ".info"


# ---- .info: ExampleInfo in protobuf text format -----------------------------
def format_info(info: dict) -> str:
    """What writeProtoToASCIIFile emits for an ExampleInfo dict ({"num_ex",
    "slot": [slot dicts]}): fields in field-number order."""
    out = []
    for s in info["slot"]:
        out.append("slot {\n  format: %s\n  id: %d\n  min_key: %d\n  max_key: %d\n"
                   "  nnz_ele: %d\n  nnz_ex: %d\n}\n"
                   % (FORMAT_NAMES[int(s["format"])], s["id"], s["min_key"], s["max_key"],
                      s["nnz_ele"], s["nnz_ex"]))
    out.append("num_ex: %d\n" % info["num_ex"])
    return "".join(out)


_TOKEN = re.compile(r"\s*([A-Za-z_][A-Za-z_0-9]*|[{}:<>]|-?[0-9][0-9A-Za-z_]*)")


def parse_info(text: str) -> dict:
    """An ExampleInfo dict from protobuf text format, whitespace-tolerant; the
    enum by name or by number.  Fields that are absent keep the proto's
    defaults (min_key: 2^64 - 1, the others 0)."""
    text = re.sub(r"#[^\n]*", "", text)
    toks, at = [], 0
    while True:
        m = _TOKEN.match(text, at)
        if not m:
            break
        toks.append(m.group(1))
        at = m.end()
    if text[at:].strip():
        raise ValueError("ExampleInfo text: cannot read %r" % text[at:at + 20].strip())
    info = {"num_ex": 0, "slot": []}
    i, cur = 0, None
    while i < len(toks):
        t = toks[i]
        if cur is not None and t in ("}", ">"):
            info["slot"].append(cur)
            cur = None
            i += 1
            continue
        if t == "slot" and cur is None:
            i += 1
            if i < len(toks) and toks[i] == ":":
                i += 1
            if i >= len(toks) or toks[i] not in ("{", "<"):
                raise ValueError("ExampleInfo text: 'slot' without a block")
            cur = {"id": 0, "format": 0, "min_key": (1 << 64) - 1, "max_key": 0, "nnz_ele": 0,
                   "nnz_ex": 0}
            i += 1
            continue
        if i + 2 >= len(toks) or toks[i + 1] != ":":
            raise ValueError("ExampleInfo text: field %r without a value" % t)
        v = toks[i + 2]
        if cur is None:
            if t != "num_ex":
                raise ValueError("ExampleInfo text: field %r" % t)
            info["num_ex"] = int(v, 0)
        elif t == "format":
            cur["format"] = _FORMAT_IDS[v] if v in _FORMAT_IDS else int(v, 0)
            if cur["format"] not in FORMAT_NAMES:
                raise ValueError("ExampleInfo text: format %r" % v)
        elif t in cur:
            cur[t] = int(v, 0)
        else:
            raise ValueError("ExampleInfo text: field %r" % t)
        i += 3
    if cur is not None:
        raise ValueError("ExampleInfo text: a slot block is not closed")
    return info


def write_info(path: str, info: dict) -> None:
    with open(path, "w") as f:
        f.write(format_info(info))


def read_info(path: str) -> dict:
    with open(path) as f:
        return parse_info(f.read())


# ---- .partition -------------------------------------------------------------
def format_partitions(parts: Sequence[Tuple[int, int]]) -> str:
    """appendPartitionInfo's lines (slot_reader.cc:112-119)."""
    return "".join("%d\t%d\n" % (int(a), int(b)) for a, b in parts)


def parse_partitions(text: str) -> List[Tuple[int, int]]:
    """assemblePartitions' reading (slot_reader.cc:294-305)."""
    out = []
    for line in text.split("\n"):
        if line == "":
            continue
        f = line.split("\t")
        if len(f) != 2:  # CHECK_EQ(2, vec.size())
            raise ValueError("partition line %r" % line)
        out.append((int(f[0]), int(f[1])))
    return out


def read_array_file(name: str) -> Tuple[bytes, Optional[List[Tuple[int, int]]]]:
    """A cache array's bytes and its partitions; a missing file is an empty
    array, a missing or empty ``.partition`` file (None) one whole-file
    stream."""
    if not os.path.exists(name):
        return b"", None
    with open(name, "rb") as f:
        data = f.read()
    parts = None
    pn = name + ".partition"
    if os.path.exists(pn) and os.path.getsize(pn):
        with open(pn) as f:
            parts = parse_partitions(f.read())
    return data, parts


# ---- the C entries ----------------------------------------------------------
def pack_bound(raw_bytes: int, part_bytes: int) -> Tuple[int, int]:
    """psg_cache_pack_bound: (cap, nparts)."""
    cap, n = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.lib().psg_cache_pack_bound(int(raw_bytes), int(part_bytes), C.byref(cap),
                                               C.byref(n)))
    return cap.value, n.value


_ELT = {_lib.PSG_CACHE_COLIDX: 8, _lib.PSG_CACHE_ROWSIZ: 2, _lib.PSG_CACHE_VALUE: 4,
        _lib.PSG_CACHE_LABEL: 4}


def mb_cache_pack(mb: Minibatch, what: int, part_bytes: int, check: bool = True):
    """psg_mb_cache_pack: (the streams back to back, [(start, size)]).  With
    ``check`` off: (status, bad_row, data, parts)."""
    L = _lib.lib()
    n = mb.rows if what in (_lib.PSG_CACHE_ROWSIZ, _lib.PSG_CACHE_LABEL) else mb.nnz
    cap, np_ = C.c_size_t(), C.c_size_t()
    rc = L.psg_cache_pack_bound(n * _ELT.get(what, 8), int(part_bytes), C.byref(cap), C.byref(np_))
    out = np.zeros(max(cap.value, 1), np.uint8)
    parts = np.zeros(2 * max(np_.value, 1), np.uint64)
    ln, got, bad = C.c_size_t(), C.c_size_t(), C.c_int64(-1)
    if rc == _lib.PSG_OK:
        rc = L.psg_mb_cache_pack(mb._h, int(what), int(part_bytes), _ptr(out), cap.value,
                                 C.byref(ln), _ptr(parts), np_.value, C.byref(got), C.byref(bad))
    data = out[:ln.value].tobytes()
    pl = [(int(parts[2 * i]), int(parts[2 * i + 1])) for i in range(got.value)]
    if not check:
        return rc, int(bad.value), data, pl
    _lib.check(rc)
    return data, pl


def _cache_array(keep: list, arr) -> "_lib.CacheArray":
    data, parts = arr if arr is not None else (b"", None)
    a = _lib.CacheArray()
    buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(0, np.uint8)
    keep.append(buf)
    a.data, a.nbytes = (buf.ctypes.data if buf.size else None), buf.size
    if parts:
        p = np.ascontiguousarray(np.array(parts, np.uint64).reshape(-1))
        keep.append(p)
        a.parts, a.nparts = p.ctypes.data_as(C.POINTER(C.c_uint64)), len(parts)
    else:
        a.parts, a.nparts = None, 0
    return a


def mb_load_cache(mb: Minibatch, files: Sequence[dict], valued: bool, check: bool = True):
    """psg_mb_load_cache.  ``files``: one dict per file with "num_ex" and, each
    optional, "colidx" / "rowsiz" / "value" / "label" as (bytes, partitions or
    None).  Returns the psg_cache_result; with ``check`` off: (status, result)."""
    keep: list = []
    arr = (_lib.CacheFile * max(len(files), 1))()
    for i, f in enumerate(files):
        arr[i].colidx = _cache_array(keep, f.get("colidx"))
        arr[i].rowsiz = _cache_array(keep, f.get("rowsiz"))
        arr[i].value = _cache_array(keep, f.get("value"))
        arr[i].label = _cache_array(keep, f.get("label"))
        arr[i].num_ex = int(f["num_ex"])
    r = _lib.CacheResult()
    rc = _lib.lib().psg_mb_load_cache(mb._h, arr, len(files), 1 if valued else 0, C.byref(r))
    mb.rows, mb.nnz = (int(r.rows), int(r.nnz)) if rc == _lib.PSG_OK else (0, 0)
    mb.n_uniq = mb.ndict = 0
    if not check:
        return rc, r
    _lib.check(rc)
    return r


def _host_streams(raw: bytes, part_bytes: int) -> Tuple[bytes, List[Tuple[int, int]]]:
    """A host array cut and compressed as psg_mb_cache_pack cuts a device one."""
    step = part_bytes if part_bytes else max(len(raw), 1)
    out, parts, at = [], [], 0
    for b in range(0, len(raw), step):
        s = compress_host(raw[b:b + step])
        out.append(s)
        parts.append((at, len(s)))
        at += len(s)
    return b"".join(out), parts


# ---- the reader -------------------------------------------------------------
class _FileWriter:
    """The cache files of one text file while it is parsed."""

    def __init__(self, prefix: str, path: str):
        self.prefix, self.path = prefix, path
        self.started = set()
        self.rows_written: Dict[int, int] = {}

    def append(self, slot_id: int, ext: str, data: bytes, parts) -> None:
        name = cache_name(self.prefix, self.path, slot_id) + ext
        first = name not in self.started
        self.started.add(name)
        with open(name, "wb" if first else "ab") as f:
            start = 0 if first else f.seek(0, os.SEEK_END)
            f.write(data)
        with open(name + ".partition", "w" if first else "a") as f:
            f.write(format_partitions([(start + a, b) for a, b in parts]))

    def pad(self, slot_id: int, upto: int) -> None:
        """Zero row sizes for the rows the slot has not seen (the reference's
        zero-padding)."""
        have = self.rows_written.get(slot_id, 0)
        if have < upto:
            s = compress_host(np.zeros(upto - have, np.uint16).tobytes())
            self.append(slot_id, ".rowsiz", s, [(0, len(s))])
        self.rows_written[slot_id] = upto


class CachedSlotReader:
    """SlotReader over text files with its cache files under ``cache_prefix``
    (a string the names are appended to, as the reference's ``cache_``), on
    the device of context ``ctx`` (a PSG_F64 context)."""

    def __init__(self, ctx, cache_prefix: str, fmt, chunk_bytes: int = DEFAULT_CHUNK_BYTES,
                 part_bytes: int = DEFAULT_PART_BYTES, skip_bad: bool = True):
        if chunk_bytes < MIN_CHUNK_BYTES:
            raise ValueError("chunk_bytes below %d" % MIN_CHUNK_BYTES)
        if part_bytes % 8:
            raise ValueError("part_bytes is no multiple of 8")
        self._ctx = ctx
        self.prefix = cache_prefix
        self.fmt = fmt
        self.valued = _format(fmt) == _lib.PSG_TEXT_LIBSVM
        self.chunk_bytes, self.part_bytes, self.skip_bad = int(chunk_bytes), int(part_bytes), skip_bad
        self._sr: Optional[SlotReader] = None
        self._tmp: Optional[Minibatch] = None
        self.paths: List[str] = []
        self.file_info: List[dict] = []
        self.info: List[dict] = []
        self.num_ex = 0
        self.hit_cache = 0
        self.bad_lines: List[Tuple[str, int]] = []
        self._labels: Dict[str, tuple] = {}

    def close(self):
        for m in (self._sr, self._tmp):
            if m is not None:
                m.close()
        self._sr = self._tmp = None

    # -- a miss: parse, pack, write
    def _chunks(self, path: str):
        """(text, final) pieces of the file, each cut after the last '\\n' at
        or before chunk_bytes; only the last is final."""
        with open(path, "rb") as f:
            carry = b""
            while True:
                buf = carry + f.read(self.chunk_bytes - len(carry))
                if len(buf) < self.chunk_bytes:
                    yield buf, True
                    return
                cut = buf.rfind(b"\n") + 1
                while cut == 0:  # a line longer than a chunk: up to its end (the parse rejects it)
                    more = f.read(self.chunk_bytes)
                    if not more:
                        yield buf, True
                        return
                    at = more.find(b"\n")
                    buf += more
                    cut = len(buf) - len(more) + at + 1 if at >= 0 else 0
                yield buf[:cut], False
                carry = buf[cut:]

    def _write_chunk(self, w: _FileWriter, sr: SlotReader, before: int) -> None:
        rows = sr.num_ex
        pb = self.part_bytes
        for s in sr.info:
            sid = s["id"]
            w.pad(sid, before)
            if sid == 0:
                w.append(0, ".value", *mb_cache_pack(sr.mb, _lib.PSG_CACHE_LABEL, pb))
                w.append(0, ".rowsiz", *_host_streams(np.ones(rows, np.uint16).tobytes(), pb))
            else:
                sr.extract(sid, self._tmp)
                for what in (_lib.PSG_CACHE_COLIDX, _lib.PSG_CACHE_ROWSIZ) + (
                        (_lib.PSG_CACHE_VALUE,) if self.valued else ()):
                    w.append(sid, _EXT[what], *mb_cache_pack(self._tmp, what, pb))
            w.rows_written[sid] = before + rows

    def _parse_file(self, path: str) -> dict:
        if self._sr is None:
            self._sr, self._tmp = SlotReader(self._ctx), Minibatch(self._ctx)
        sr, w = self._sr, _FileWriter(self.prefix, path)
        info = {"num_ex": 0, "slot": []}
        line0 = 0
        for text, final in self._chunks(path):
            if text:
                sr.read(text, self.fmt, self.skip_bad, final)
                self.bad_lines += [(path, line0 + b) for b in sr.bad_lines]
                line0 += text.count(b"\n") + (0 if text.endswith(b"\n") else 1)
                if sr.num_ex:
                    self._write_chunk(w, sr, info["num_ex"])
                    info = merge_example_info(info, sr.example_info())
        for sid in list(w.rows_written):
            w.pad(sid, info["num_ex"])
        write_info(info_name(self.prefix, path), info)  # last: an interrupted run is no hit
        return info

    def read(self, paths: Sequence[str]) -> List[dict]:
        """SlotReader::read over ``paths``: a file whose ``.info`` exists is a
        hit, every other file is parsed and cached.  Returns ``info``, the
        slots of all the files merged (the label slot 0 first)."""
        self.paths, self.file_info, self.hit_cache = [str(p) for p in paths], [], 0
        self.bad_lines, self._labels = [], {}
        total = {"num_ex": 0, "slot": []}
        for p in self.paths:
            name = info_name(self.prefix, p)
            if os.path.exists(name):  # readFileToProto succeeds: the data is in the cache
                fi = read_info(name)
                self.hit_cache += 1
            else:
                fi = self._parse_file(p)
            self.file_info.append(fi)
            total = merge_example_info(total, fi)
        self.info, self.num_ex = total["slot"], total["num_ex"]
        return self.info

    def example_info(self) -> dict:
        return {"num_ex": self.num_ex, "slot": list(self.info)}

    def slots(self) -> List[int]:
        return [s["id"] for s in self.info if s["id"] != 0]

    # -- index() / offset() / value() of one slot over every file
    def _label(self, path: str):
        if path not in self._labels:
            self._labels[path] = read_array_file(cache_name(self.prefix, path, 0) + ".value")
        return self._labels[path]

    def extract(self, slot_id: int, minibatch: Minibatch) -> None:
        """One slot of all the files as ``minibatch`` (of the same context):
        num_ex rows in the files' order; a file without the slot gives empty
        rows."""
        files = []
        for p, fi in zip(self.paths, self.file_info):
            stem = cache_name(self.prefix, p, slot_id)
            value = read_array_file(stem + ".value")
            if not self.valued:
                if any(b for _, b in (value[1] if value[1] is not None else [(0, len(value[0]))])):
                    raise _lib.PSGError(_lib.PSG_ERR_SIZE,
                                        f"{stem}.value holds values, the group is binary")
                value = None  # a valued group's count is checked by the load
            files.append({"colidx": read_array_file(stem + ".colidx"),
                          "rowsiz": read_array_file(stem + ".rowsiz"), "value": value,
                          "label": self._label(p), "num_ex": fi["num_ex"]})
        mb_load_cache(minibatch, files, self.valued)
