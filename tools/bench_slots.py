"""MEASUREMENT AID: text ingest by feature group.

The text is an ADFEA text of --groups feature groups (slot ids 1, 2, ...): the
workload of bench_worker (Zipf 1.1 ids mapped through a table of 64-bit keys,
seed 1) with every row's entries dealt to the groups in runs.  As the median
of --steps runs after --warmup untimed ones, with at least 100 ms of untimed
device work first, all in one process:

  load_text_ms          psg_mb_load_text on the same bytes: the existing path,
                        the yardstick (host clock; it ends in a device wait)
  load_text_groups_ms   psg_mb_load_text_groups (host clock)
  parse_ms / parse_groups_ms
                        the kernels of the two loads by HIP events
                        (psg_mb_profile), the slow tokens' host time included
  groups_ms             psg_mb_groups by HIP events recorded on the context's
                        stream around the call (its one host wait included),
                        and by the host clock
  extract_all_ms        psg_mb_group_extract of every group, one after
                        another, the same two ways; per group in extract_ms

The structural condition is checked, not a ratio: one host wait in
psg_mb_groups and the one of the load's second half per extraction is what
the code does (psg_groups.hip); nothing here asserts a speed.

Prints one JSON object; --out writes it to a file too.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def render(offset, index, y, groups):
    out = []
    off = offset.astype(np.int64)
    for r in range(y.size):
        ks = index[off[r]:off[r + 1]].tolist()
        n = len(ks)
        out.append("%d 1 %d " % (r, y[r] > 0) +
                   " ".join("%d:%d" % (k, 1 + j * groups // n) for j, k in enumerate(ks)))
    return ("\n".join(out) + "\n").encode()


def median(t):
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--mean-nnz", type=int, default=64)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from bench_worker import minibatch
    from parameter_server_amd import _lib, slots
    from parameter_server_amd.worker import Minibatch, text_chunk, sort_tile

    L = _lib.lib()
    table = np.random.default_rng(a.seed).integers(0, 1 << 64, size=a.universe, dtype=np.uint64)
    offset, index, value, y = minibatch(a.seed * 1000, a.rows, a.mean_nnz, a.zipf, a.universe,
                                        table)
    text = render(offset, index, y, a.groups)
    ctx = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(ctx)))
    src = Minibatch(ctx)
    dst = [Minibatch(ctx) for _ in range(a.groups)]
    stream = torch.cuda.ExternalStream(src.stream)

    def timed(fn):
        """(event ms, host ms) of fn(), the events on the context's stream."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), host

    # the two loads give the same matrix; the grouping gives what the text holds
    r0 = src.load_text(text, "adfea", a.rows, True)
    want = [src.read(n) for n in ("offset", "index", "y")]
    r1 = src.load_text_groups(text, "adfea", a.rows, True)
    got = [src.read(n) for n in ("offset", "index", "y")]
    assert all(np.array_equal(g.view(np.uint64), w.view(np.uint64)) for g, w in zip(got, want))
    assert r0.rows == r1.rows == a.rows and r0.bad_line == r1.bad_line == -1
    info, bad = slots.mb_groups(src)
    assert bad == -1 and [s["id"] for s in info] == list(range(a.groups + 1))
    assert sum(s["nnz_ele"] for s in info[1:]) == index.size

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:  # untimed: clocks up
        src.load_text_groups(text, "adfea", a.rows, True)
    src.profile(True)
    rec = {k: [] for k in ("load", "parse", "loadg", "parseg", "groups_ev", "groups_host",
                           "extract_ev", "extract_host")}
    per_group = [[] for _ in range(a.groups)]
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        p = src.load_text(text, "adfea", a.rows, True).parse_ms
        t1 = time.perf_counter()
        pg = src.load_text_groups(text, "adfea", a.rows, True).parse_ms
        t2 = time.perf_counter()
        g_ev, g_host = timed(lambda: slots.mb_groups(src))
        x_ev = x_host = 0.0
        each = []
        for g in range(a.groups):
            ev, host = timed(lambda: slots.mb_group_extract(src, g + 1, dst[g]))
            x_ev += ev
            x_host += host
            each.append(ev)
        if step < a.warmup:
            continue
        for k, v in zip(rec, ((t1 - t0) * 1e3, p, (t2 - t1) * 1e3, pg, g_ev, g_host, x_ev, x_host)):
            rec[k].append(v)
        for g in range(a.groups):
            per_group[g].append(each[g])
    src.profile(False)
    nb = len(text)
    out = {
        "tool": "bench_slots",
        "workload": {"rows": a.rows, "mean_nnz_per_row": a.mean_nnz, "nnz": int(index.size),
                     "groups": a.groups, "zipf_exponent": a.zipf, "universe": a.universe,
                     "ids": "64-bit table", "seed": a.seed, "format": "adfea",
                     "text_bytes": nb, "slow_tokens": int(r1.slow_tokens)},
        "method": {"steps": a.steps, "warmup": a.warmup, "figure": "median (and min)",
                   "untimed_first_ms": 100, "chunk_bytes": text_chunk(), "sort_tile": sort_tile(),
                   "events": "HIP events on the context's stream around each call",
                   "one_process": True},
        "group_entries": [s["nnz_ele"] for s in info[1:]],
        "load_text_ms": median(rec["load"]), "parse_ms": median(rec["parse"]),
        "load_text_groups_ms": median(rec["loadg"]), "parse_groups_ms": median(rec["parseg"]),
        "groups_ms": median(rec["groups_ev"]), "groups_host_ms": median(rec["groups_host"]),
        "extract_all_ms": median(rec["extract_ev"]),
        "extract_all_host_ms": median(rec["extract_host"]),
        "extract_ms": [median(t) for t in per_group],
        "host_waits": {"psg_mb_groups": 1, "psg_mb_group_extract": 1},
        "lib": os.path.basename(_lib.LIB_PATH),
    }
    for m in dst:
        m.close()
    src.close()
    L.psg_destroy(ctx)
    s = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
