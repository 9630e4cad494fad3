"""MEASUREMENT AID: the direct scorer (psg_ftrl_score_dev, psg_ftrlm_score_dev)
against the predict chain it stands beside.

Prints one JSON object.  Workload: bench_worker's minibatch (--rows x
--mean-nnz entries, Zipf ids mapped through a table of 64-bit keys) against a
model that holds every key of the table, as a scalar model and as a sweep of
each --models m.  Timed span, from "loaded" to "Xw ready", by a pair of HIP
events on the minibatch's stream:
  predict   uniq (sort, run lengths, its host read of n_uniq) + pull of the
            unique keys + localize + times / times_rows
  score     the one call, in float64 and in float32
The minibatch is loaded again (untimed) before every timed span, the two paths
alternate, --warmup untimed rounds come first (each is two loads and both
paths: well over 100 ms), and every figure is the median of --steps.  The
float64 scores are compared with the predict chain's by bits."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ftrl_multi import Events, spread  # noqa: E402
from bench_worker import minibatch  # noqa: E402

PARAM = dict(alpha=0.1, beta=1.0, lambda1=0.01, lambda2=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="8,32")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--mean-nnz", type=int, default=64)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from parameter_server_amd import _lib
    from parameter_server_amd.ftrl import FTRLModel, FTRLMultiModel
    from parameter_server_amd.worker import FTRLMultiWorker, FTRLWorker, score_tile

    rng = np.random.default_rng(a.seed)
    table = rng.integers(0, 1 << 64, size=a.universe, dtype=np.uint64)
    batches = [minibatch(a.seed * 1000 + b, a.rows, a.mean_nnz, a.zipf, a.universe, table)
               for b in range(a.batches)]
    keys = np.unique(table)
    cnt = np.zeros(keys.size, np.uint64)
    ev = Events()
    results = []
    for m in [0] + [int(x) for x in a.models.split(",") if x]:
        w = rng.standard_normal((keys.size, max(m, 1))) * 0.1
        if m == 0:
            model = FTRLModel(0, capacity_hint=keys.size)
            model.restore(keys, cnt, cnt, w[:, 0], w[:, 0])
            wk = FTRLWorker(model)
        else:
            model = FTRLMultiModel([PARAM] * m, 0, capacity_hint=keys.size)
            model.restore(keys, cnt, cnt, w, w)
            wk = FTRLMultiWorker(model)
        del w
        mb = wk.mb

        def predict():
            if m == 0:
                wk._predict_loaded()
            else:
                _, pulled = wk._pull(False)
                mb.times_rows(pulled, m, mb.scratch(wk._FILTER, 8 * mb.rows * m))

        def xw():
            if m == 0:
                return mb.read("xw")
            return mb.read_scratch(wk._FILTER, np.float64, mb.rows * m).copy()

        paths = {"predict": predict,
                 "score_f64": lambda: wk._score_loaded(np.float64),
                 "score_f32": lambda: wk._score_loaded(np.float32)}
        ms = {k: [] for k in paths}
        same = True
        for i in range(a.warmup + a.steps):
            batch = batches[i % a.batches]
            got = {}
            for name, work in paths.items():
                mb.load(*batch)  # untimed; every path starts from "loaded"
                t = ev.time(mb.stream, work)
                if i >= a.warmup:
                    ms[name].append(t)
                if i == a.warmup and name != "score_f32":
                    got[name] = xw()
            if got:
                same = same and got["predict"].tobytes() == got["score_f64"].tobytes()
        r = {k: spread(v) for k, v in ms.items()}
        results.append({
            "models": m or "scalar",
            "tile_entries": {"f64": score_tile(m, np.float64), "f32": score_tile(m, np.float32)},
            "ms": r,
            "predict_over_score_f64": r["predict"]["median"] / r["score_f64"]["median"],
            "predict_over_score_f32": r["predict"]["median"] / r["score_f32"]["median"],
            "entries_per_s_score_f64": batches[0][1].size / (r["score_f64"]["median"] * 1e-3),
            "score_f64_bits_equal_predict": bool(same),
        })
        wk.close()
        model.close()
    print(json.dumps({
        "tool": "bench_score",
        "workload": {"rows": a.rows, "mean_nnz_per_row": a.mean_nnz,
                     "nnz": int(batches[0][1].size), "zipf_exponent": a.zipf,
                     "universe": a.universe, "model_keys": int(keys.size), "seed": a.seed,
                     "batches": a.batches},
        "method": {"timer": "HIP events on the minibatch's stream, loaded -> Xw ready",
                   "steps": a.steps, "warmup_rounds": a.warmup, "figure": "median",
                   "paths": "alternating, a fresh load before each"},
        "not_measured": ["other row lengths", "a cold table", "a table far larger than L2 "
                         "read uniformly (Zipf ids keep the hot keys cached)"],
        "results": results,
        "lib": os.path.basename(_lib.LIB_PATH),
    }))


if __name__ == "__main__":
    main()
