"""MEASUREMENT AID: one pass of Darling for m settings (darling_pass_rows)
against m passes of the scalar device path (darling_pass), one worker.

Prints one JSON object and writes it to --out (profiles/darling_multi.json).
For the binary and the valued matrix and every m of --models:

  rows_pass_ms     one darling_pass_rows over --blocks key blocks: gradients,
                   the server's update and update_dual of every block for all
                   m settings, enqueued, then one device wait;
  scalar_passes_ms m darling_pass runs one after the other, one per setting,
                   on one scalar worker and server channel, then one wait;
  ratio            rows_pass_ms / scalar_passes_ms (below 1: the sweep wins).

Host clock around enqueue + wait; medians over --steps timed repeats after
--prewarm-ms of untimed repeats (the clocks rise over the first ~25 ms of
work, as bench.py's prewarm notes) and --warmup more.  The workload is
tools/bench_darling_worker.py's minibatch and blocks.  Every pass is a real
solver pass from the state the last one left, with a KKT threshold that
inactivates nothing, so every (key, model) stays live.  Not measured: more
than one worker (the fold through RowMergePlan), other row lengths.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_worker import minibatch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--mean-nnz", type=int, default=64)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--models", default="1,4,8,16,32")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prewarm-ms", type=float, default=100.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "darling_multi.json"))
    a = ap.parse_args()

    import torch
    from parameter_server_amd import (DarlingMultiServer, DarlingMultiWorker, DarlingWorker, _lib,
                                      darling_pass_rows)
    from parameter_server_amd.darling import darling_pass
    from parameter_server_amd.kv_vector import KVVector, Message

    table = np.random.default_rng(a.seed).integers(0, 1 << 64, size=a.universe, dtype=np.uint64)
    offset, index, value, y = minibatch(a.seed * 1000, a.rows, a.mean_nnz, a.zipf, a.universe,
                                        table)
    dic = np.unique(index)
    nd = dic.size
    cut = np.linspace(0, nd, a.blocks + 1).astype(np.int64)
    blocks = [(int(dic[cut[b]]), int(dic[cut[b + 1]]) if cut[b + 1] < nd else (1 << 64) - 1)
              for b in range(a.blocks)]
    wait = torch.cuda.synchronize

    def setting(j):
        return dict(eta=0.8, lambda_=0.05 * (j + 1), kkt_filter_threshold=1e20, delta_max=5.0)

    def timed(fn):
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < a.prewarm_ms:
            fn()
            wait()
        ms = []
        for i in range(a.warmup + a.steps):
            wait()
            t0 = time.perf_counter()
            fn()
            wait()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    ctx = KVVector(0, _lib.PSG_F64)
    results = []
    for binary in (True, False):
        val = None if binary else value
        sw = DarlingWorker(ctx._h, 1.0, 5.0)
        sw.load(offset, index, val, y, dic)
        chl = 1 if binary else 2
        ctx.setValue(Message(key=dic, key_channel=chl))
        ctx.set_value_array(chl, np.zeros(nd))
        _lib.check(ctx._L.psg_darling_init(ctx._h, chl, 1.0))
        clock = [10]

        def scalar_passes(m):
            for j in range(m):
                clock[0] = darling_pass(ctx, [sw], chl, clock[0], blocks, setting(j))

        one = timed(lambda: scalar_passes(1))
        for m in [int(x) for x in a.models.split(",")]:
            srv = DarlingMultiServer(ctx._h, dic, [setting(j) for j in range(m)], 1.0)
            mw = DarlingMultiWorker(ctx._h, m, 1.0, 5.0)
            mw.load(offset, index, val, y, dic)
            rows_ms = timed(lambda: darling_pass_rows(srv, [mw], blocks))
            scal_ms = timed(lambda: scalar_passes(m))
            ctx.dev_status()
            results.append({"binary": binary, "m": m, "rows_pass_ms": rows_ms[0],
                            "rows_pass_ms_min_max": rows_ms[1:], "scalar_passes_ms": scal_ms[0],
                            "scalar_passes_ms_min_max": scal_ms[1:],
                            "ratio": rows_ms[0] / scal_ms[0],
                            "rows_pass_over_one_scalar_pass": rows_ms[0] / one[0]})
            print(json.dumps(results[-1]), file=sys.stderr, flush=True)
            mw.close()
            srv.close()
            del srv, mw
            torch.cuda.empty_cache()
        results.append({"binary": binary, "m": 0, "one_scalar_pass_ms": one[0]})
        sw.close()
    out = {
        "tool": "bench_darling_multi",
        "workload": {"rows": a.rows, "mean_nnz_per_row": a.mean_nnz, "nnz": int(index.size),
                     "zipf_exponent": a.zipf, "universe": a.universe, "ndict": int(nd),
                     "blocks": a.blocks, "workers": 1, "seed": a.seed},
        "method": {"steps": a.steps, "warmup": a.warmup, "prewarm_ms": a.prewarm_ms,
                   "timer": "host clock around enqueue + device wait", "figure": "median"},
        "results": results,
        "not_measured": ["more than one worker (RowMergePlan fold, gather_rows_dev)",
                         "other row lengths and dictionary sizes"],
        "lib": os.path.basename(_lib.LIB_PATH),
    }
    ctx.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
