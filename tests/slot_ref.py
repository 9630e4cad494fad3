"""The reference's grouped text path restated in Python, for the tests of the
text ingest by feature group: FileLineReader's chop
(src/util/filelinereader.cc:34-42), ExampleParser::parseAdfea / parseLibsvm
with ignore_fea_slot_ = false (src/data/example_parser.cc:84-160), toProto's
bookkeeping and info() (:38-82) and SlotReader's per-slot storage with its
zero padding (src/data/slot_reader.cc:146-166,211-219).  Numbers go through
libc by tests/text_ref.py's helpers.  The defined deviations of include/psg.h
are restated too: a line holding a slot id outside [1, 4095] is rejected, and
a rejected line ends the parse.  Unpinned: the reference's parser is not
compiled in."""
import re

import numpy as np

import text_ref as T

ADFEA, LIBSVM = T.ADFEA, T.LIBSVM
SLOT_MAX = 4096
DENSE, SPARSE, SPARSE_BINARY = 1, 2, 3


def chop(line):
    """The line as the parser sees it: its '\\n', then at most one '\\r', gone."""
    if line.endswith(b"\n"):
        line = line[:-1]
    if line.endswith(b"\r"):
        line = line[:-1]
    return line


def fast_slot(t):
    return re.fullmatch(rb"[0-9]{1,4}", t) is not None


def walk_adfea(line):
    """The tokens of one ADFEA line in order, as (kind, token, value, ok):
    kind in "skip", "label", "key", "slot"; ok False: the token rejects the
    line.  Ends after the first such token."""
    out = []
    for i, t in enumerate(T.tokens_of(chop(line), ADFEA)):
        if i < 2:
            out.append(("skip", t, None, True))
            continue
        if i == 2:
            v, ok = T.strtoi32(t)
            out.append(("label", t, 1.0 if v > 0 else -1.0, ok))
        elif i % 2 == 1:
            v, ok = T.strtou64(t)
            out.append(("key", t, v, ok))
        else:
            v, ok = T.strtoi32(t)
            out.append(("slot", t, v, ok and 1 <= v < SLOT_MAX))
        if not out[-1][3]:
            break
    return out


def parse_line(line, fmt):
    """(y, [(slot, key, val or None), ...]) or None: the line is rejected."""
    if fmt == LIBSVM:  # its delimiters hold '\\r' and '\\n': the chop changes nothing
        r = T.parse_line(line, LIBSVM)
        if r is None:
            return None
        return r[0], [(1, k, v) for k, v in zip(r[1], r[2])]
    if len(line) >= T.MAX_LINE - 1 or b"\0" in line:
        return None
    toks = walk_adfea(line)
    if len(toks) < 3 or not all(t[3] for t in toks):
        return None
    y, key, ent = toks[2][2], None, []
    for kind, _, v, _ in toks[3:]:
        if kind == "key":
            key = v
        else:
            ent.append((v, key, None))
    return y, ent


def parse(text, fmt, max_rows=None, final=True):
    """(offset, index, value or None, y, slot, rows, consumed, bad_line)."""
    offset, index, value, y, slot = [0], [], [], [], []
    consumed, bad = 0, -1
    for line in T.lines_of(text, final):
        if max_rows is not None and len(y) >= max_rows:
            break
        consumed += len(line)
        r = parse_line(line, fmt)
        if r is None:
            bad = len(y)
            break
        y.append(r[0])
        for s, k, v in r[1]:
            slot.append(s)
            index.append(k)
            value.append(v)
        offset.append(len(index))
    val = np.array(value, dtype=np.float32).astype(np.float64) if fmt == LIBSVM else None
    return (np.array(offset, dtype=np.uint64), np.array(index, dtype=np.uint64), val,
            np.array(y, dtype=np.float64), np.array(slot, dtype=np.uint16), len(y), consumed, bad)


def slow_tokens(text, fmt, max_rows=None, final=True):
    """The tokens outside the fast grammar up to the token that rejects a
    line, as psg_text_parse_groups_host counts them."""
    if fmt == LIBSVM:
        return T.slow_tokens(text, fmt, max_rows, final, stop_at_bad=True)
    n = 0
    for row, line in enumerate(T.lines_of(text, final)):
        if max_rows is not None and row >= max_rows:
            break
        if len(line) >= T.MAX_LINE - 1 or b"\0" in line:
            break
        toks = walk_adfea(line)
        for kind, t, _, _ in toks:
            if kind == "label":
                n += len(t) > T.MAX_FIELD or not T.fast_label(t)
            elif kind == "key":
                n += len(t) > T.MAX_FIELD or not T.fast_key(t)
            elif kind == "slot":
                n += not fast_slot(t)
        if len(toks) < 3 or not toks[-1][3]:
            break
    return n


def skip_parse(text, fmt, final=True):
    """SlotReader's handling (slot_reader.cc:148): a rejected line is skipped
    and has no effect.  (rows as [(y, entries)], the skipped lines' numbers)."""
    rows, bad = [], []
    for i, line in enumerate(T.lines_of(text, final)):
        r = parse_line(line, fmt)
        if r is None:
            bad.append(i)
        else:
            rows.append(r)
    return rows, bad


def runs_of(entries):
    """The slots of one example as parseAdfea adds them: a new slot whenever
    the id changes (example_parser.cc:150-154)."""
    runs = []
    for s, k, v in entries:
        if not runs or runs[-1][0] != s:
            runs.append((s, []))
        runs[-1][1].append((k, v))
    return runs


def split_rows(rows):
    """The rows in which a slot id occurs in two separate runs."""
    out = []
    for r, (_, ent) in enumerate(rows):
        ids = [s for s, _ in runs_of(ent)]
        if len(ids) != len(set(ids)):
            out.append(r)
    return out


def info(rows, fmt):
    """toProto's bookkeeping and info() over `rows` ([(y, entries)]): the slot
    dicts in ascending id order."""
    st = {}
    for _, ent in rows:
        runs = runs_of(ent)
        if fmt == LIBSVM and not runs:
            runs = [(1, [])]  # parseLibsvm adds slot 1 to every example
        for s, kv in runs:
            t = st.setdefault(s, {"min_key": (1 << 64) - 1, "max_key": 0, "nnz_ele": 0, "nnz_ex": 0})
            for k, _ in kv:
                t["min_key"] = min(t["min_key"], k)
                t["max_key"] = max(t["max_key"], (k + 1) & ((1 << 64) - 1))
            t["nnz_ex"] += 1
            t["nnz_ele"] += len(kv)
    out = []
    if rows:
        out.append({"id": 0, "format": DENSE, "min_key": 0, "max_key": 1, "nnz_ele": len(rows),
                    "nnz_ex": len(rows)})
    for s in sorted(st):
        if st[s]["nnz_ele"]:
            out.append(dict(st[s], id=s, format=SPARSE if fmt == LIBSVM else SPARSE_BINARY))
    return out


def storage(rows, slot_id, fmt):
    """SlotReader::offset / index / value of one slot: row_siz with its zero
    padding as offsets, col_idx, val (None for ADFEA), and y."""
    offset, index, value = [0], [], []
    for _, ent in rows:
        for s, k, v in ent:
            if s == slot_id:
                index.append(k)
                value.append(v)
        offset.append(len(index))
    val = np.array(value, dtype=np.float32).astype(np.float64) if fmt == LIBSVM else None
    return (np.array(offset, dtype=np.uint64), np.array(index, dtype=np.uint64), val,
            np.array([y for y, _ in rows], dtype=np.float64))
