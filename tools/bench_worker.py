"""MEASUREMENT AID: the device-resident worker step (psg_mb_*, FTRLWorker).

Prints one JSON object: the time of each stage of the step -- sort,
run_length, localize, count_keys, times, logit, trans_times -- taken with HIP
events that the library records around the stage's launches
(psg_mb_profile / psg_mb_stage_ms), and the host time of a whole
FTRLWorker.step (which ends in a device wait), its psg_mb_load part apart
(the minibatch crosses PCIe from pageable memory there).  Every figure is the
median over --steps timed steps after --warmup untimed ones over the same
minibatch shapes.

The workload is seeded and stated in the output: rows, mean entries per row,
the Zipf exponent of the ids, the number of distinct ids and the longest run
of the first minibatch.  Ids are the ranks of a Zipf draw mapped through a
random table of 64-bit keys (every radix pass runs), or with --dense-ids the
ranks themselves (the passes over constant digits are skipped).

The sort's traffic is counted from its shape: the count pass reads the keys
(8 B per pair), the scatter reads the pairs (12 B; 8 B in the first pass,
whose positions are implicit) and writes them (12 B).  Its rate is set
against the copy ceiling recorded in profiles/ (the `roofline` block of
--ceiling-from, measured with tools/copybw on an MI355X).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAM = dict(alpha=0.1, beta=1.0, lambda1=0.01, lambda2=0.1)


def minibatch(seed, rows, mean, zipf_a, universe, table):
    rng = np.random.default_rng(seed)
    nnz = rows * mean
    cdf = np.cumsum(np.arange(1, universe + 1, dtype=np.float64) ** -zipf_a)
    rank = np.searchsorted(cdf, rng.random(nnz) * cdf[-1]).astype(np.uint64)
    index = rank if table is None else table[rank.astype(np.int64)]
    lens = rng.multinomial(nnz, np.full(rows, 1.0 / rows))
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    value = rng.standard_normal(nnz) * 0.05
    y = np.where(rng.random(rows) < 0.5, 1.0, -1.0)
    return offset, index, value, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--mean-nnz", type=int, default=64)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--dense-ids", action="store_true")
    ap.add_argument("--tail-feature-freq", type=int, default=0)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ceiling-from", default=os.path.join(ROOT, "profiles", "r06_bench.json"))
    a = ap.parse_args()

    from parameter_server_amd import _lib
    from parameter_server_amd.ftrl import FTRLModel
    from parameter_server_amd.worker import FTRLWorker, sort_tile

    table = None
    if not a.dense_ids:
        table = np.random.default_rng(a.seed).integers(0, 1 << 64, size=a.universe,
                                                       dtype=np.uint64)
    batches = [minibatch(a.seed * 1000 + b, a.rows, a.mean_nnz, a.zipf, a.universe, table)
               for b in range(a.batches)]
    index0 = batches[0][1]
    counts = np.unique(index0, return_counts=True)[1]
    differ = int(np.bitwise_or.reduce(index0) ^ np.bitwise_and.reduce(index0))
    passes = sum(1 for d in range(8) if (differ >> (8 * d)) & 0xFF)
    nnz = index0.size

    model = FTRLModel(0, capacity_hint=min(a.universe, 1 << 23))
    model.setLearningRate(PARAM["alpha"], PARAM["beta"])
    model.setPenalty(PARAM["lambda1"], PARAM["lambda2"])
    worker = FTRLWorker(model, tail_feature_freq=a.tail_feature_freq)
    for i in range(a.warmup):  # untimed: every shape, the model's growth, code objects
        worker.step(*batches[i % a.batches])
    worker.mb.profile(True)
    stages = {s: [] for s in _lib.MB_STAGES}
    step_ms, load_ms, objv = [], [], 0.0
    for i in range(a.steps):
        off, idx, val, y = batches[i % a.batches]
        t0 = time.perf_counter()
        worker.mb.load(off, idx, val, y)
        t1 = time.perf_counter()
        load_ms.append((t1 - t0) * 1e3)
        t0 = time.perf_counter()
        objv, _ = worker.step(off, idx, val, y)
        ms = worker.mb.stage_ms()  # waits for the push as well
        step_ms.append((time.perf_counter() - t0) * 1e3)
        for s, v in ms.items():
            stages[s].append(v)
    med = {s: float(np.median(v)) for s, v in stages.items()}
    lo = {s: float(np.min(v)) for s, v in stages.items()}
    sort_bytes = passes * 32 * nnz - (4 * nnz if passes else 0)
    ceiling = None
    try:
        ceiling = json.load(open(a.ceiling_from))["roofline"]["measured_copy_GBps"]
    except Exception:
        pass
    sort_gbps = sort_bytes / (med["sort"] * 1e-3) / 1e9 if med["sort"] > 0 else None
    out = {
        "tool": "bench_worker",
        "workload": {"rows": a.rows, "mean_nnz_per_row": a.mean_nnz, "nnz": int(nnz),
                     "zipf_exponent": a.zipf, "universe": a.universe,
                     "ids": "dense ranks" if a.dense_ids else "64-bit table",
                     "n_uniq": int(counts.size), "longest_run": int(counts.max()),
                     "median_run": float(np.median(counts)), "seed": a.seed,
                     "tail_feature_freq": a.tail_feature_freq, "batches": a.batches},
        "method": {"steps": a.steps, "warmup": a.warmup, "stage_timer": "HIP events",
                   "step_timer": "host clock around step + device wait", "figure": "median"},
        "sort": {"tile_pairs": sort_tile(), "digit_bits": 8, "passes_run": passes,
                 "passes_skipped": 8 - passes, "bytes_moved": int(sort_bytes),
                 "GBps": sort_gbps, "copy_ceiling_GBps": ceiling,
                 "copy_ceiling_source": os.path.relpath(a.ceiling_from, ROOT),
                 "fraction_of_copy_ceiling": (sort_gbps / ceiling
                                              if sort_gbps and ceiling else None),
                 "pairs_per_s": nnz / (med["sort"] * 1e-3) if med["sort"] > 0 else None},
        "stage_ms_median": med,
        "stage_ms_min": lo,
        "device_ms_sum_of_stages": float(sum(med.values())),
        "load_ms_median": float(np.median(load_ms)),
        "step_ms_median": float(np.median(step_ms)),
        "step_ms_min": float(np.min(step_ms)),
        "last_objv": objv,
        "lib": os.path.basename(_lib.LIB_PATH),
    }
    worker.close()
    model.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
