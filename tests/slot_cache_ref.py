"""TEST INFRASTRUCTURE: SlotReader's cache arrays restated in plain Python.

``read_one_file`` is readOneFile's slot filling (src/data/slot_reader.cc:
142-220) over the grouped host parse (``parse_groups_skipping``, which has
SlotReader's skip of a rejected line): per slot the col_idx / row_siz / val
arrays with the zero padding of :158-161 and :215-218, dumped every
``dump_rows`` rows as the periodic check does (:169-201) and once at the end.
``assemble`` is index() / offset() / value() (:234-290) over several files.

One difference from the reference, as the product defines it: the final
padding goes to every slot that has been written, also to one whose arrays
are empty after a periodic dump.  The reference skips such a slot (:213), its
row sizes stay short of num_ex and its own offset() then fails
CHECK_EQ(os.size(), num_ex + 1).  The recorded cases avoid that state.
"""
import numpy as np

from parameter_server_amd import slots

EXTS = ("colidx", "rowsiz", "value")
DTYPES = {"colidx": np.uint64, "rowsiz": np.uint16, "value": np.float32}


def partitions(raw: bytes, part_bytes: int):
    """psg_mb_cache_pack's cut of a raw array."""
    if not raw:
        return []
    step = part_bytes if part_bytes else len(raw)
    return [raw[b:b + step] for b in range(0, len(raw), step)]


def cache_arrays(offset, index, value, y):
    """The four raw arrays of psg_mb_cache_pack for a CSR minibatch."""
    offset = np.asarray(offset, np.uint64)
    d = np.diff(offset.astype(np.int64))
    out = {"colidx": np.asarray(index, np.uint64).tobytes(),
           "rowsiz": d.astype(np.uint16).tobytes(),
           "label": np.asarray(y, np.float64).astype(np.float32).tobytes()}
    if value is not None:
        out["value"] = np.asarray(value, np.float64).astype(np.float32).tobytes()
    return out


def read_one_file(text: bytes, fmt: str, dump_rows=None):
    """(num_ex, {slot id: {"colidx" / "rowsiz" / "value": [raw partition bytes]}}).
    Every dump appends one partition to each of the slot's three files, an
    empty one included (compressTo of an empty array: 0 bytes)."""
    offset, index, value, y, slot, _bad = slots.parse_groups_skipping(text, fmt)
    libsvm = value is not None
    rows = y.size
    cur, total, files = {}, {}, {}

    def vslot(s):
        if s not in cur:
            cur[s] = {"colidx": [], "rowsiz": [], "value": []}
            total.setdefault(s, 0)
        return cur[s]

    def dump():
        for s in sorted(cur):
            v = cur[s]
            if not v["rowsiz"] and not v["value"]:
                continue
            f = files.setdefault(s, {e: [] for e in EXTS})
            for e in EXTS:
                f[e].append(np.asarray(v[e], DTYPES[e]).tobytes())
                v[e] = []

    def push(s, keys, vals, num_ex):
        v = vslot(s)
        v["colidx"] += keys
        v["value"] += vals
        v["rowsiz"] += [0] * (num_ex - total[s])  # the zero padding
        v["rowsiz"].append(max(len(keys), len(vals)) & 0xffff)  # pushBack into SArray<uint16>
        total[s] = num_ex + 1

    for r in range(rows):
        push(0, [], [float(np.float32(y[r]))], r)
        b, e = int(offset[r]), int(offset[r + 1])
        if libsvm:  # parseLibsvm adds slot 1 to every example
            push(1, [int(k) for k in index[b:e]], [float(x) for x in value[b:e]], r)
        else:
            i = b
            while i < e:  # the runs of one slot id
                j = i
                while j < e and slot[j] == slot[i]:
                    j += 1
                push(int(slot[i]), [int(k) for k in index[i:j]], [], r)
                i = j
        if dump_rows and (r + 1) % dump_rows == 0 and r + 1 < rows:
            dump()
    for s in total:
        if total[s] < rows:
            vslot(s)["rowsiz"] += [0] * (rows - total[s])
            total[s] = rows
    dump()
    return rows, files


def assemble(per_file, slot_id: int, valued: bool):
    """index() / offset() / value() and the labels over the files: per_file is
    a list of (num_ex, files) as read_one_file returns them.  A file without
    the slot gives num_ex empty rows.  Returns offset, index, value or None, y."""
    idx, siz, val, lab = [], [], [], []
    for num_ex, files in per_file:
        f = files.get(slot_id)
        if f is None:
            siz.append(np.zeros(num_ex, np.uint16))
        else:
            idx += [np.frombuffer(p, np.uint64) for p in f["colidx"]]
            siz += [np.frombuffer(p, np.uint16) for p in f["rowsiz"]]
            val += [np.frombuffer(p, np.float32) for p in f["value"]]
        if 0 in files:
            lab += [np.frombuffer(p, np.float32) for p in files[0]["value"]]
    cat = lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t)  # noqa: E731
    offset = np.concatenate([np.zeros(1, np.uint64), np.cumsum(cat(siz, np.uint64), dtype=np.uint64)])
    return (offset, cat(idx, np.uint64), cat(val, np.float64) if valued else None,
            cat(lab, np.float64))
