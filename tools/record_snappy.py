#!/usr/bin/env python3
"""Record real snappy streams into tests/golden/snappy_pin/.

Compresses every case of tests/pin_cases.py snappy_cases() with the locally
installed google snappy (its C interface, snappy-c.h, loaded by ctypes; nothing
is downloaded) and stores the streams as data-only fixtures (numpy .npz: one
uint8 array per case and a JSON `meta` holding the library's file name and
version, each input's SHA-256 and length, and the element tally of each
stream, with the table form's count of copies it cannot place, npend).  Every stream is decoded back by the library and by the oracle's
orc_snappy_uncompress before it is written.  Run by hand, on the CPU, when the
cases change; no test calls it.  A fixture is never edited to fit: if a
decoder disagrees with one, the code is what changes.

    python tools/record_snappy.py            record
    python tools/record_snappy.py --seam     search the kTabMax pair's n
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pin_cases as P  # noqa: E402
from snappy_lib import Snappy  # noqa: E402

MAX_BYTES = 128 * 1024       # a file, as tools/record_reference.py
MAX_TOTAL = 320 * 1024       # all snappy fixtures
K_TAB_MAX = 4096             # psg_snappy.hip kTabMax


def seam(S):
    """The largest n whose keys-below-2^40 stream has <= kTabMax elements and
    the smallest n whose stream has more."""
    count = {}
    for n in range(2000, 2500):
        count[n] = P.snappy_tally(S.compress(P.le_bytes(P.keys_below(40002, n, 40))))["elements"]
    le = max(n for n, c in count.items() if c <= K_TAB_MAX)
    gt = min(n for n, c in count.items() if c > K_TAB_MAX)
    print("largest n with <= %d elements: %d (%d); smallest n with more: %d (%d)"
          % (K_TAB_MAX, le, count[le], gt, count[gt]))


def main():
    import oracle_py as O
    try:
        S = Snappy()
    except OSError as e:
        sys.exit("%s: install google snappy (libsnappy) to record" % e)
    if "--seam" in sys.argv[1:]:
        return seam(S)
    source = {"library": S.file, "version": S.version, "call": "snappy_compress (snappy-c.h), "
              "which is snappy::RawCompress"}
    groups = {g: ({"source": source, "cases": {}}, {}) for g in P.SNAPPY_GROUPS}
    print("%-18s %7s %7s %8s %7s %8s %7s %7s" % ("case", "bytes", "stream", "elements", "copy-1",
                                                 "high-bit", "run", "npend"))
    for c in P.snappy_cases():
        stream = S.compress(c.data)
        assert S.uncompress(stream) == c.data, c.name
        assert O.snappy_uncompress(stream) == c.data, c.name
        t = P.snappy_tally(stream)
        assert t["uncompressed"] == len(c.data)
        meta, arrays = groups[c.group]
        meta["cases"][c.name] = {"input_sha256": c.digest(), "uncompressed": len(c.data), "tally": t}
        arrays[c.name] = np.frombuffer(stream, np.uint8)
        print("%-18s %7d %7d %8d %7d %8d %7d %7s" % (
            c.name, len(c.data), len(stream), t["elements"], t["copy1"], t["copy1_high"],
            t["longest_copy_run"], "-" if t["table_npend"] is None else t["table_npend"]))
    for g, (meta, arrays) in groups.items():
        P.save_fixture(g, meta, arrays, P.SNAPPY_GOLDEN)
    total = 0
    for f in sorted(os.listdir(P.SNAPPY_GOLDEN)):
        size = os.path.getsize(os.path.join(P.SNAPPY_GOLDEN, f))
        total += size
        print("%-28s %7d bytes" % (f, size))
        assert size <= MAX_BYTES, f
    print("%-28s %7d bytes" % ("total", total))
    assert total <= MAX_TOTAL


if __name__ == "__main__":
    main()
