"""MEASUREMENT AID: the exact AUC of a sweep (psg_auc_exact_rows_dev) against m
scalar calls (psg_auc_exact_dev) over the same data.

Writes one JSON object (--out, default profiles/auc_exact_rows.json) and prints
it.  For each m of --models: one ``psg_auc_exact_rows_dev`` over --rows
examples of m seeded normal predictions, row-major as the worker writes them,
and m ``psg_auc_exact_dev`` calls over the columns of the same data
de-interleaved beforehand; the de-interleave (a strided device copy) is timed
on its own and is part of neither figure.  Both sides are timed in the same
run, alternating, with HIP events on the context's stream after at least
100 ms of untimed calls of the same shapes; every figure is the median over
--reps timed calls, with the smallest and largest kept.  The events span each
call's allocation, its host waits (two per call: 2 for the rows form, 2 m for
the scalar calls) and its free, so a figure is the time a caller sees on an
otherwise idle stream, not a sum of kernel times.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auc_exact_rows.json"))
    a = ap.parse_args()

    import torch
    from parameter_server_amd import _lib
    from parameter_server_amd.auc import exact_auc_dev, exact_auc_rows_dev
    from parameter_server_amd.worker import Minibatch, sort_tile

    if not torch.cuda.is_available():
        raise SystemExit("bench_auc_exact_rows.py needs a GPU: a CPU run measures nothing")
    L = _lib.lib()
    ctx = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(ctx)))
    mb = Minibatch(ctx)  # for the context's stream
    stream = torch.cuda.ExternalStream(mb.stream)
    rng = np.random.default_rng(a.seed)
    n = a.rows

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(prefix, t):
        return {prefix + "_ms_median": float(np.median(t)), prefix + "_ms_min": float(np.min(t)),
                prefix + "_ms_max": float(np.max(t))}

    results = []
    for m in a.models:
        y_h = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        p_h = rng.normal(0, 2.0, (n, m)) + 0.8 * y_h[:, None]
        y, p = torch.from_numpy(y_h).cuda(), torch.from_numpy(p_h).cuda()
        cols = torch.empty((m, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        got = {}

        def rows_call():
            got["rows"] = exact_auc_rows_dev(ctx, y.data_ptr(), p.data_ptr(), n, m, mb.stream)

        def scalar_calls():
            got["scalar"] = np.array([exact_auc_dev(ctx, y.data_ptr(), cols.data_ptr() + 8 * n * j,
                                                    n, mb.stream) for j in range(m)])

        def deinterleave():
            with torch.cuda.stream(stream):
                cols.copy_(p.t())

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:  # untimed: code objects, the allocator's pools
            deinterleave()
            rows_call()
            scalar_calls()
            stream.synchronize()
        t_rows, t_scalar, t_split = [], [], []
        for _ in range(a.reps):  # alternating
            t_split.append(timed(deinterleave))
            t_rows.append(timed(rows_call))
            t_scalar.append(timed(scalar_calls))
        # the passes the rows form ran: the digits in which any two keys of any column differ
        b = p_h.view(np.uint64).reshape(-1)
        key = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
        differ = int(np.bitwise_or.reduce(key) ^ np.bitwise_and.reduce(key))
        passes = sum(1 for d in range(8) if (differ >> (8 * d)) & 255)
        # bytes from the shape, per element: the key kernel 8 + 8; a pass 8 (count) + 12 + 12
        # (the last writes no key: - 8); the area 4 + 8 (the gathered label) + 1 + 1
        total = n * m
        nbytes = total * (16 + passes * 32 - 8 + 14) + 4 * 256 * 3 * passes * m * -(-n // sort_tile())
        r, s = float(np.median(t_rows)), float(np.median(t_scalar))
        row = {"m": m, "passes": passes, "bytes_from_shape": int(nbytes),
               "rows_gb_per_s": nbytes / r / 1e6, "scalar_over_rows": s / r,
               "bits_equal": bool(np.array_equal(got["rows"].view(np.uint64),
                                                 got["scalar"].view(np.uint64)))}
        row.update(stats("rows_call", t_rows))
        row.update(stats("scalar_calls", t_scalar))
        row.update(stats("deinterleave", t_split))
        results.append(row)
        del y, p, cols
    out = {
        "tool": "bench_auc_exact_rows",
        "method": {"timer": "HIP events on the context's stream around the call(s)",
                   "untimed_first_ms": 100, "reps": a.reps, "figure": "median, min and max kept",
                   "order": "de-interleave, rows and scalar alternate within one run",
                   "deinterleave": "timed on its own, part of neither figure"},
        "rows": n, "seed": a.seed, "by_m": results,
        "not_tried": ["kernel-level times (no profiler run)", "the label in the payload",
                      "other transpose tile heights"],
        "lib": os.path.basename(_lib.LIB_PATH),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    mb.close()
    L.psg_destroy(ctx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
