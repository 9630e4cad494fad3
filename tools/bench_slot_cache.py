"""MEASUREMENT AID: the SlotReader cache.

The data set is bench_slots' (an ADFEA text of --groups feature groups over
bench_worker's Zipf workload), split into --files text files.  "All groups
resident" (every group extracted into its own minibatch) is timed three ways,
each the median of --steps runs after --warmup untimed ones, by the host clock
around work that ends in a device wait, all in one process after at least
100 ms of untimed device work:

  text_ms   SlotReader.read of the whole text plus extract of every group:
            the only path before the cache, the yardstick
  cold_ms   CachedSlotReader.read over an empty cache (parse, pack, write)
            plus extract of every group
  warm_ms   a new CachedSlotReader over the filled cache (read the .info
            files) plus extract of every group (read files, psg_mb_load_cache);
            warm_host_only_ms is the same with psg_mb_load_cache left out

warm_ms is taken at each --part-bytes value (the raw bytes per partition the
writer cuts), with the cache's size, and so is cold_ms.  The arrays of the
three paths are compared bit for bit before anything is timed.  Nothing here
asserts a speed.

Prints one JSON object; --out writes it to a file too.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stat(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--mean-nnz", type=int, default=64)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--part-bytes", type=int, nargs="+",
                    default=[4 << 10, 16 << 10, 64 << 10, 256 << 10, 1 << 20])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from bench_slots import render
    from bench_worker import minibatch
    from parameter_server_amd import _lib, slot_cache, slots
    from parameter_server_amd.worker import Minibatch

    L = _lib.lib()
    table = np.random.default_rng(a.seed).integers(0, 1 << 64, size=a.universe, dtype=np.uint64)
    offset, index, value, y = minibatch(a.seed * 1000, a.rows, a.mean_nnz, a.zipf, a.universe,
                                        table)
    work = tempfile.mkdtemp(prefix="bench_slot_cache_")
    paths, texts = [], []
    per = (a.rows + a.files - 1) // a.files
    for f in range(a.files):
        lo, hi = f * per, min((f + 1) * per, a.rows)
        b, e = int(offset[lo]), int(offset[hi])
        t = render(offset[lo:hi + 1] - offset[lo], index[b:e], y[lo:hi], a.groups)
        p = os.path.join(work, "part-%d.adfea" % f)
        with open(p, "wb") as fh:
            fh.write(t)
        paths.append(p)
        texts.append(t)
    text = b"".join(texts)

    ctx = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(ctx)))
    ids = list(range(1, a.groups + 1))
    dst = [Minibatch(ctx) for _ in ids]
    sr = slots.SlotReader(ctx)

    def from_text():
        sr.read(text, "adfea")
        for g, m in zip(ids, dst):
            sr.extract(g, m)

    def prefix_of(pb):
        return os.path.join(work, "cache_%d" % pb) + os.sep

    def cold(pb):
        shutil.rmtree(prefix_of(pb), ignore_errors=True)
        os.makedirs(prefix_of(pb))
        rd = slot_cache.CachedSlotReader(ctx, prefix_of(pb), "adfea", part_bytes=pb)
        rd.read(paths)
        assert rd.hit_cache == 0
        for g, m in zip(ids, dst):
            rd.extract(g, m)
        rd.close()

    def warm(pb):
        rd = slot_cache.CachedSlotReader(ctx, prefix_of(pb), "adfea", part_bytes=pb)
        rd.read(paths)
        assert rd.hit_cache == len(paths)
        for g, m in zip(ids, dst):
            rd.extract(g, m)
        rd.close()

    def arrays():
        return [[m.read(n).tobytes() for n in ("offset", "index", "y")] for m in dst]

    from_text()
    want = arrays()
    sizes = {}
    for pb in a.part_bytes:
        cold(pb)
        assert arrays() == want
        warm(pb)
        assert arrays() == want
        names = os.listdir(prefix_of(pb))
        sizes[pb] = {"bytes": sum(os.path.getsize(os.path.join(prefix_of(pb), n)) for n in names),
                     "files": len(names)}

    def timed(fn, *args):
        t = []
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            fn(*args)  # ends in a device wait: the last extract's
            if step >= a.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        return stat(t)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:  # untimed: clocks up
        from_text()
    text_ms = timed(from_text)
    warm_ms = {pb: timed(warm, pb) for pb in a.part_bytes}
    # the host's share of the warm path: everything but psg_mb_load_cache
    load = slot_cache.mb_load_cache
    slot_cache.mb_load_cache = lambda *args, **kw: None
    warm_host_ms = {pb: timed(warm, pb) for pb in a.part_bytes}
    slot_cache.mb_load_cache = load
    cold_ms = {pb: timed(cold, pb) for pb in a.part_bytes}
    text_again_ms = timed(from_text)  # the spread of the yardstick within the process
    best = min(a.part_bytes, key=lambda pb: warm_ms[pb]["median"])
    out = {
        "tool": "bench_slot_cache",
        "workload": {"rows": a.rows, "mean_nnz_per_row": a.mean_nnz, "nnz": int(index.size),
                     "groups": a.groups, "files": a.files, "zipf_exponent": a.zipf,
                     "universe": a.universe, "ids": "64-bit table", "seed": a.seed,
                     "format": "adfea", "text_bytes": len(text)},
        "method": {"steps": a.steps, "warmup": a.warmup, "figure": "median, min, max in ms",
                   "clock": "host clock around calls that end in a device wait",
                   "untimed_first_ms": 100, "one_process": True,
                   "file_system": "the machine's temporary directory (page cache warm)",
                   "checked": "offset, index and y of every group equal on all three paths"},
        "text_ms": text_ms, "text_again_ms": text_again_ms,
        "cold_ms": {str(pb): cold_ms[pb] for pb in a.part_bytes},
        "warm_ms": {str(pb): warm_ms[pb] for pb in a.part_bytes},
        "warm_host_only_ms": {str(pb): warm_host_ms[pb] for pb in a.part_bytes},
        "cache": {str(pb): dict(sizes[pb], of_text=sizes[pb]["bytes"] / len(text))
                  for pb in a.part_bytes},
        "fastest_part_bytes": best,
        "default_part_bytes": slot_cache.DEFAULT_PART_BYTES,
        "lib": os.path.basename(_lib.LIB_PATH),
    }
    sr.close()
    for m in dst:
        m.close()
    L.psg_destroy(ctx)
    shutil.rmtree(work, ignore_errors=True)
    s = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
