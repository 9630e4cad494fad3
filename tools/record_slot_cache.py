#!/usr/bin/env python3
"""Records tests/golden/slot_cache/: SlotReader's cache files in the
reference's format for three small texts, with the arrays they must load to.

Every stream is snappy_compress (the installed google snappy, through
tests/snappy_lib.py) of a whole array, as SArray::compressTo makes it; the
arrays are readOneFile's (tests/slot_cache_ref.py).  Each case is recorded
twice: "single", one dump at the end of the file, and "multi", a periodic
dump every few rows, each dump one ``start\\tsize`` line of the array's
``.partition`` file.  The expected offset / index / value / y come from
another restatement, tests/slot_ref.py's storage() over the concatenated
text.

One .npz per case and form:
  texts        the files' texts, uint8, back to back; text_len their lengths
  num_ex       the files' example counts
  slots        the feature slots of the set
  f<i>_s<id>_<ext>        a cache file's bytes (uint8); the label slot is s0
  f<i>_s<id>_<ext>_parts  its .partition lines as (start, size) rows
  s<id>_offset / _index / _value,  y    what the set must load to
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import slot_cache_ref as R  # noqa: E402
import slot_ref as S  # noqa: E402
from snappy_lib import Snappy  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "slot_cache")

ADFEA3 = (b"a 1 1 100:2 101:2 7:3\n"
          b"b 1 0 102:2\n"
          b"c 1 1 8:3 9:3\n"
          b"d 1 1 103:2 18446744073709551615:5 10:3\n"   # slot 5 first appears here
          b"e 1 -1 5000:5\n"
          b"f 1 1\n"                                        # a row without an entry
          b"g 1 0 104:2 105:2 106:2 11:3\n"
          b"h 1 1 107:2 12:3 5001:5 5002:5\n")
LIBSVM = (b"1 3:0.5 7:1.25 9:-2\n"
          b"-1 2:1\n"
          b"1\n"                                            # a label alone: an empty row of slot 1
          b"0.5 1:3 1:4 4000000000:0.125\n"
          b"-1 8:1e-3 9:16777217\n"
          b"1 5:2\n")
TWO_A = (b"a 1 1 1:2 2:2 30:4\n"
         b"b 1 0 3:2\n"
         b"c 1 1 31:4 32:4 4:2\n")
TWO_B = (b"d 1 0 5:2 6:2\n"                                 # slot 4 is absent from this file
         b"e 1 1 7:2\n")

CASES = {
    "adfea3": ("adfea", [ADFEA3], 3),
    "libsvm": ("libsvm", [LIBSVM], 2),
    "adfea_two_files": ("adfea", [TWO_A, TWO_B], 2),
}


def record(name, fmt, texts, dump_rows, snappy):
    sfmt = S.ADFEA if fmt == "adfea" else S.LIBSVM
    out = {"texts": np.frombuffer(b"".join(texts), np.uint8),
           "text_len": np.array([len(t) for t in texts], np.uint64)}
    num_ex, slots = [], set()
    for i, t in enumerate(texts):
        n, files = R.read_one_file(t, fmt, dump_rows)
        num_ex.append(n)
        slots |= set(s for s in files if s != 0)
        for s, f in files.items():
            for ext in R.EXTS:
                data, parts = b"", []
                for raw in f[ext]:
                    z = snappy.compress(raw) if raw else b""  # compressTo of an empty array
                    parts.append((len(data), len(z)))
                    data += z
                out["f%d_s%d_%s" % (i, s, ext)] = np.frombuffer(data, np.uint8)
                out["f%d_s%d_%s_parts" % (i, s, ext)] = np.array(parts, np.uint64).reshape(-1, 2)
    out["num_ex"] = np.array(num_ex, np.uint64)
    out["slots"] = np.array(sorted(slots), np.int64)
    rows, bad = S.skip_parse(b"".join(texts), sfmt)
    assert not bad
    for s in sorted(slots):
        offset, index, value, y = S.storage(rows, s, sfmt)
        out["s%d_offset" % s], out["s%d_index" % s], out["y"] = offset, index, y
        if value is not None:
            out["s%d_value" % s] = value
    return out


def main():
    snappy = Snappy()
    os.makedirs(GOLDEN, exist_ok=True)
    total = 0
    for name, (fmt, texts, dump_rows) in CASES.items():
        for form, dr in (("single", None), ("multi", dump_rows)):
            path = os.path.join(GOLDEN, "%s_%s.npz" % (name, form))
            np.savez(path, **record(name, fmt, texts, dr, snappy))
            total += os.path.getsize(path)
            print(path, os.path.getsize(path))
    print("libsnappy %s, %d bytes in all" % (snappy.version, total))


if __name__ == "__main__":
    main()
