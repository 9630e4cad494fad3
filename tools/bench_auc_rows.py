"""MEASUREMENT AID: the row-valued AUC (psg_auc_rows_add_dev) against m scalar
adds (psg_auc_add_dev) over the same data.

Writes one JSON object (--out, default profiles/auc_rows.json) and prints it.
For each m of --models: one ``psg_auc_rows_add_dev`` of --rows examples of m
predictions onto a table that --fill earlier adds have filled, and m
``psg_auc_add_dev`` calls over the de-interleaved columns of the same data
onto m scalar histograms filled the same way.  The de-interleave is done once,
before any timing.  Both sides are timed in the same run, alternating, with HIP
events on the context's stream after at least 100 ms of untimed work of the
same shapes; every figure is the median over --reps timed calls.  A rows add
waits on the host once and the m scalar adds m times (each reads its batch's
key span): the events span those waits, so a figure is the time a caller sees
on an otherwise idle stream, not a sum of kernel times.
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
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--goodness", type=int, default=100000)
    ap.add_argument("--fill", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sigma", type=float, default=2.0, help="spread of the predictions")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auc_rows.json"))
    a = ap.parse_args()

    import torch
    from parameter_server_amd import _lib
    from parameter_server_amd.auc import AUC, AUCRows
    from parameter_server_amd.worker import Minibatch

    if not torch.cuda.is_available():
        raise SystemExit("bench_auc_rows.py needs a GPU: a CPU run measures nothing")
    L = _lib.lib()
    ctx = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(ctx)))
    mb = Minibatch(ctx)  # for the context's stream
    stream = torch.cuda.ExternalStream(mb.stream)
    rng = np.random.default_rng(a.seed)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    results = []
    for m in a.models:
        # fill + 1 batches: labels [rows], predictions [rows, m] and, de-interleaved, [m, rows]
        ys, ps, cols = [], [], []
        for _ in range(a.fill + 1):
            y = np.where(rng.random(a.rows) < 0.5, 1.0, -1.0)
            p = rng.normal(0, a.sigma, (a.rows, m)) + 0.8 * y[:, None]
            ys.append(torch.from_numpy(y).cuda())
            ps.append(torch.from_numpy(p).cuda())
            cols.append(torch.from_numpy(np.ascontiguousarray(p.T)).cuda())
        torch.cuda.synchronize()
        rows_h = AUCRows(ctx, m, a.goodness)
        scalar_h = [AUC(ctx, a.goodness) for _ in range(m)]

        def add_rows(i):
            rows_h.add_dev(ys[i].data_ptr(), ps[i].data_ptr(), a.rows, mb.stream)

        def add_scalar(i):
            for j, h in enumerate(scalar_h):
                h.add_dev(ys[i].data_ptr(), cols[i].data_ptr() + 8 * a.rows * j, a.rows, mb.stream)

        def fill(add, handles):
            for h in handles:
                h.clear()
            for i in range(a.fill):
                add(i)
            stream.synchronize()

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:  # untimed: code objects, every buffer's growth
            fill(add_rows, [rows_h])
            add_rows(a.fill)
            fill(add_scalar, scalar_h)
            add_scalar(a.fill)
            stream.synchronize()
        t_rows, t_scalar = [], []
        for _ in range(a.reps):  # alternating, each onto its own filled table
            fill(add_rows, [rows_h])
            t_rows.append(timed(lambda: add_rows(a.fill)))
            fill(add_scalar, scalar_h)
            t_scalar.append(timed(lambda: add_scalar(a.fill)))
        same = all(all(np.array_equal(x, z) for x, z in zip(rows_h.data(j), scalar_h[j].data()))
                   for j in range(m))
        resident = sum(int(np.union1d(d[0], d[2]).size) for d in (rows_h.data(j) for j in range(m)))
        r, s = float(np.median(t_rows)), float(np.median(t_scalar))
        results.append({"m": m, "rows_add_ms_median": r, "rows_add_ms_min": float(np.min(t_rows)),
                        "rows_add_ms_max": float(np.max(t_rows)), "scalar_adds_ms_median": s,
                        "scalar_adds_ms_min": float(np.min(t_scalar)),
                        "scalar_adds_ms_max": float(np.max(t_scalar)),
                        "scalar_over_rows": s / r, "resident_entries_after": resident,
                        "tables_equal": bool(same)})
        rows_h.close()
        for h in scalar_h:
            h.close()
        del ys, ps, cols
    out = {
        "tool": "bench_auc_rows",
        "method": {"timer": "HIP events on the context's stream around the call(s)",
                   "untimed_first_ms": 100, "reps": a.reps, "figure": "median",
                   "order": "rows and scalar alternate within one run"},
        "rows": a.rows, "goodness": a.goodness, "earlier_adds": a.fill,
        "prediction_sigma": a.sigma, "seed": a.seed, "by_m": results,
        "not_tried": ["the wide case (timed nowhere: m + 1 host waits)",
                      "kernel-level times (no profiler run)"],
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
