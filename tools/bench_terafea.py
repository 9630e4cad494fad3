"""MEASUREMENT AID: TERAFEA text ingest.

The workload of bench_slots (bench_worker's Zipf 1.1 rows over a table of
64-bit keys, seed 1) written as TERAFEA: every key's top 10 bits are one of
--groups groups, the keys of a line in their drawn order.  The yardstick is
psg_mb_load_text_groups on ADFEA text of the same rows and entries, the two
loads alternating in one loop.  Medians of --steps runs after --warmup
untimed ones, at least 100 ms of untimed device work first:

  load_terafea_ms / load_adfea_ms    the whole call, host clock (it ends in a
                                     device wait)
  parse_terafea_ms / parse_adfea_ms  the loads' kernels by HIP events
                                     (psg_mb_profile)
  load_beta_ms / parse_beta_ms       the same with the beta entry too (the
                                     finish pass then searches every entry's row)
  ratio_*                            TERAFEA over ADFEA: what the sort, the
                                     check and the shuffle cost
  host_twin_ms                       psg_text_parse_terafea_host, both calls
  row_classes                        the share of rows sorted inside one tile,
                                     cut by a tile edge, longer than a tile

The stages come from the profiler in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_terafea.py --loads 20
  python tools/bench_terafea.py --stats DIR --out profiles/terafea.json
--stats adds, per kernel of the load, the mean time of one launch, and for the
sort and finish kernels their algorithmic bytes (16 and 18 per entry) over
that time as a share of --hbm-peak.  Nothing here asserts a speed.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STAGES = {"tokenise": ("count_kernel", "chunk_scan_kernel", "class_kernel", "row_scan_kernel",
                       "emit_kernel", "patch_kernel", "line_kernel", "verdict_kernel"),
          "group0_check": ("check_kernel",), "tile_sort": ("tile_kernel",),
          "cut_rows": ("edge_kernel<false>",), "long_rows": ("edge_kernel<true>",),
          "finish": ("finish_kernel", "shift_kernel")}


def render(offset, keys, y, adfea):
    off, out = offset.astype(np.int64), []
    for r in range(y.size):
        ks = keys[off[r]:off[r + 1]].tolist()
        if adfea:
            out.append("%d 1 %d " % (r, y[r] > 0) + " ".join("%d:%d" % (k, k >> 54) for k in ks))
        else:
            out.append("%d %d | " % (y[r] > 0, r) + " ".join(map(str, ks)))
    return ("\n".join(out) + "\n").encode()


def kernel_means(path):
    """kernel name -> mean ns per launch, from rocprofv3's kernel_stats.csv."""
    out = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            out[row["Name"]] = float(row["AverageNs"])
    return out


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
    ap.add_argument("--loads", type=int, default=0, help="only this many loads: the profiled run")
    ap.add_argument("--stats", default=None, help="the profiled run's output directory")
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from bench_worker import minibatch
    from parameter_server_amd import _lib, slots
    from parameter_server_amd.worker import Minibatch, terafea_tile, text_chunk

    L = _lib.lib()
    table = np.random.default_rng(a.seed).integers(0, 1 << 64, size=a.universe, dtype=np.uint64)
    table = (table & np.uint64((1 << 54) - 1)) | (
        (np.arange(a.universe, dtype=np.uint64) % np.uint64(a.groups) + np.uint64(1)) << np.uint64(54))
    offset, keys, _, y = minibatch(a.seed * 1000, a.rows, a.mean_nnz, a.zipf, a.universe, table)
    tera, adfea = render(offset, keys, y, False), render(offset, keys, y, True)
    ctx = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(ctx)))
    mb = Minibatch(ctx)
    if a.loads:
        for _ in range(a.loads):
            mb.load_terafea(tera, True, False, a.rows, True)
        mb.close()
        L.psg_destroy(ctx)
        return

    t0 = time.perf_counter()
    host = slots.parse_text_groups_host(tera, "terafea", a.rows, True, True, False)
    host_ms = (time.perf_counter() - t0) * 1e3
    r = mb.load_terafea(tera, True, False, a.rows, True)
    assert (r.rows, r.nnz, r.bad_line) == (a.rows, keys.size, -1)
    assert all(np.array_equal(mb.read(n), w) for n, w in zip(("offset", "index", "slot"),
                                                             (host[0], host[1], host[4])))
    T = terafea_tile()
    lo, hi = offset[:-1].astype(np.int64), offset[1:].astype(np.int64)
    long_ = hi - lo > T
    cut = ~long_ & (hi > lo) & (lo // T != (hi - 1) // T)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:  # untimed: clocks up
        mb.load_terafea(tera, True, False, a.rows, True)
    mb.profile(True)
    rec = {k: [] for k in ("load_terafea_ms", "parse_terafea_ms", "load_adfea_ms", "parse_adfea_ms",
                           "load_beta_ms", "parse_beta_ms")}
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        pt = mb.load_terafea(tera, True, False, a.rows, True).parse_ms
        t1 = time.perf_counter()
        pa = mb.load_text_groups(adfea, "adfea", a.rows, True).parse_ms
        t2 = time.perf_counter()
        pb = mb.load_terafea(tera, True, True, a.rows, True).parse_ms
        t3 = time.perf_counter()
        if step >= a.warmup:
            for k, v in zip(rec, ((t1 - t0) * 1e3, pt, (t2 - t1) * 1e3, pa, (t3 - t2) * 1e3, pb)):
                rec[k].append(v)
    mb.profile(False)
    med = {k: float(np.median(v)) for k, v in rec.items()}
    out = {
        "tool": "bench_terafea",
        "workload": {"rows": a.rows, "mean_nnz_per_row": a.mean_nnz, "nnz": int(keys.size),
                     "groups": a.groups, "zipf_exponent": a.zipf, "universe": a.universe,
                     "seed": a.seed, "flags": "shuffle", "terafea_bytes": len(tera),
                     "adfea_bytes": len(adfea), "slow_tokens": int(r.slow_tokens)},
        "method": {"steps": a.steps, "warmup": a.warmup, "figure": "median",
                   "untimed_first_ms": 100, "chunk_bytes": text_chunk(), "terafea_tile": T,
                   "alternating": "terafea, adfea, terafea with beta in one loop",
                   "one_process": True},
        **med,
        "ratio_load": med["load_terafea_ms"] / med["load_adfea_ms"],
        "ratio_parse": med["parse_terafea_ms"] / med["parse_adfea_ms"],
        "terafea_text_bytes_per_s": len(tera) / (med["load_terafea_ms"] * 1e-3),
        "host_twin_ms": host_ms,
        "row_classes": {"in_tile": float(1 - long_.mean() - cut.mean()), "cut": float(cut.mean()),
                        "long": float(long_.mean())},
        "stages": "not taken",
        "lib": os.path.basename(_lib.LIB_PATH),
    }
    if a.stats:
        ns = kernel_means(a.stats)
        pick = lambda names: {k: v for k, v in ns.items() if any("::" + n in k for n in names)}
        out["stages"] = {s: pick(names) for s, names in STAGES.items()}
        out["stage_ns"] = {s: sum(v.values()) for s, v in out["stages"].items()}
        n = float(keys.size)
        for s, per in (("tile_sort", 16.0), ("finish", 18.0)):
            if out["stage_ns"][s]:
                out[s + "_share_of_hbm_peak"] = per * n / (out["stage_ns"][s] * 1e-9) / a.hbm_peak
        out["hbm_peak_bytes_per_s"] = a.hbm_peak
    mb.close()
    L.psg_destroy(ctx)
    s = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    print(s)


if __name__ == "__main__":
    main()
