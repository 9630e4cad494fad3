"""MEASUREMENT AID: device-resident evaluation (psg_auc_*, psg_auc_exact_dev).

Writes one JSON object (--out, default profiles/auc.json), prints it, and
puts a line for it into the profile index (--index):

* one ``psg_auc_add_dev`` of --rows examples at --goodness onto a histogram
  that --fill earlier adds of other examples have filled, with the resident
  distinct-key count next to it;
* one ``psg_auc_exact_dev`` over --exact-n examples.

Both are timed with HIP events on the context's stream, after at least 100 ms
of untimed work of the same shapes; every figure is the median over --reps
timed calls.  An add waits on the host once (it reads the batch's key span),
and psg_auc_exact_dev allocates its buffers and waits twice: the events span
those waits, so the figures are the time of the call as a caller sees it on
an otherwise idle stream, not a sum of kernel times.

Bytes are counted from the shapes, as DESIGN.md 4.8 (a) does for the sort:
a radix pass reads the keys (8 B per item), reads the pairs (12 B; 8 B in the
first pass) and writes them (12 B).  An add further moves, per item: the key
kernel (8 + 8), the rebase (8 + 8), the run heads (count 8; emit 8 + 8 + 4 +
4), the counters (16 cleared; 4 + 4 + 8 read) and the union's run side (8 +
8 + 4 + 1 written, 1 + 4 + 4 scanned, up to 8 + 16 + 24 moved); and per
resident entry 24 B read and 24 B written (the table is rewritten by every
add).  The binary searches' reads are not counted.

The add is set next to the worker step's sum of stage times recorded in
profiles/worker_step.json (tools/bench_worker.py, the same 65,536 rows).
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


def passes_of(span):
    return sum(1 for d in range(8) if (span >> (8 * d)) != 0)


def sort_bytes(passes, n):
    return passes * 32 * n - (4 * n if passes else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--goodness", type=int, default=100000)
    ap.add_argument("--fill", type=int, default=64)
    ap.add_argument("--exact-n", type=int, default=4194304)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sigma", type=float, default=2.0, help="spread of the predictions")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auc.json"))
    ap.add_argument("--index", default=os.path.join(ROOT, "profiles", "INDEX.md"))
    ap.add_argument("--step-from", default=os.path.join(ROOT, "profiles", "worker_step.json"))
    a = ap.parse_args()

    import torch
    from parameter_server_amd import _lib
    from parameter_server_amd.auc import AUC, exact_auc_dev
    from parameter_server_amd.worker import Minibatch, sort_tile

    if not torch.cuda.is_available():
        raise SystemExit("bench_auc.py needs a GPU: a CPU run measures nothing")
    L = _lib.lib()
    ctx = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(ctx)))
    mb = Minibatch(ctx)  # for the context's stream
    stream = torch.cuda.ExternalStream(mb.stream)

    rng = np.random.default_rng(a.seed)

    def examples(n):
        y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        return y, rng.normal(0, a.sigma, n) + 0.8 * y

    host = [examples(a.rows) for _ in range(a.fill + 1)]
    devs = [(torch.from_numpy(y).cuda(), torch.from_numpy(p).cuda()) for y, p in host]
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    auc = AUC(ctx, a.goodness)

    def fill():
        auc.clear()
        for y, p in devs[:a.fill]:
            auc.add_dev(y.data_ptr(), p.data_ptr(), a.rows, mb.stream)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:  # untimed: code objects, every buffer's growth
        fill()
        auc.add_dev(devs[-1][0].data_ptr(), devs[-1][1].data_ptr(), a.rows, mb.stream)
        stream.synchronize()
    add_ev, add_host = [], []
    for _ in range(a.reps):
        fill()
        stream.synchronize()
        ev, ho = timed(lambda: auc.add_dev(devs[-1][0].data_ptr(), devs[-1][1].data_ptr(),
                                           a.rows, mb.stream))
        add_ev.append(ev)
        add_host.append(ho)
    # what the timed add met, and what it left
    fill()
    before = auc.data()
    resident_before = int(np.union1d(before[0], before[2]).size)
    auc.add_dev(devs[-1][0].data_ptr(), devs[-1][1].data_ptr(), a.rows, mb.stream)
    after = auc.data()
    resident_after = int(np.union1d(after[0], after[2]).size)
    value = auc.evaluate()
    with np.errstate(all="ignore"):
        keys = np.trunc(host[-1][1] * float(a.goodness)).astype(np.int64)
    span = int(keys.max()) - int(keys.min())
    passes = passes_of(span)
    runs = int(np.unique(keys).size)
    n = a.rows
    per_item = (8 + 8) + (8 + 8) + 8 + (8 + 8 + 4 + 4) + 16 + (4 + 4 + 8) + (8 + 8 + 4 + 1) + \
        (1 + 4 + 4)
    add_bytes = sort_bytes(passes, n) + per_item * n + (8 + 16 + 24) * runs + 48 * resident_before
    add_ms = float(np.median(add_ev))

    # the exact AUC
    ye, pe = examples(a.exact_n)
    tye, tpe = torch.from_numpy(ye).cuda(), torch.from_numpy(pe).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    exact = None
    while exact is None or time.perf_counter() - t0 < 0.1:
        exact = exact_auc_dev(ctx, tye.data_ptr(), tpe.data_ptr(), a.exact_n, mb.stream)
    ex_ev, ex_host = [], []
    for _ in range(max(3, a.reps // 2)):
        ev, ho = timed(lambda: exact_auc_dev(ctx, tye.data_ptr(), tpe.data_ptr(), a.exact_n,
                                             mb.stream))
        ex_ev.append(ev)
        ex_host.append(ho)
    kb = np.where(pe == 0, np.uint64(0), pe.view(np.uint64))  # the sort key of psg_auc.hip
    kb = np.where(kb >> np.uint64(63) != 0, ~kb, kb | np.uint64(1 << 63))
    differ = int(np.bitwise_or.reduce(kb) ^ np.bitwise_and.reduce(kb))
    ex_passes = sum(1 for d in range(8) if (differ >> (8 * d)) & 0xFF)
    m = a.exact_n
    exact_bytes = sort_bytes(ex_passes, m) + (8 + 8) * m + 8 * m + (4 + 8) * m + \
        (4 + 8 + 4) * m + 4 * m
    ex_ms = float(np.median(ex_ev))

    step_sum = None
    try:
        step_sum = json.load(open(a.step_from))["device_ms_sum_of_stages"]
    except Exception:
        pass
    out = {
        "tool": "bench_auc",
        "method": {"timer": "HIP events on the context's stream around the call",
                   "untimed_first_ms": 100, "reps": a.reps, "figure": "median"},
        "add": {
            "rows": n, "goodness": a.goodness, "earlier_adds": a.fill,
            "prediction_sigma": a.sigma, "seed": a.seed,
            "resident_distinct_keys_before": resident_before,
            "resident_distinct_keys_after": resident_after,
            "batch_distinct_keys": runs, "batch_key_span": span,
            "radix_passes_run": passes, "sort_tile_pairs": sort_tile(),
            "ms_median": add_ms, "ms_min": float(np.min(add_ev)),
            "ms_max": float(np.max(add_ev)),
            "host_ms_median": float(np.median(add_host)),
            "bytes_from_shape": int(add_bytes),
            "GBps_from_shape": add_bytes / (add_ms * 1e-3) / 1e9,
            "examples_per_s": n / (add_ms * 1e-3),
            "worker_step_sum_of_stages_ms": step_sum,
            "worker_step_source": os.path.relpath(a.step_from, ROOT),
            "fraction_of_worker_step": add_ms / step_sum if step_sum else None,
            "evaluate_by_key": value,
        },
        "exact": {
            "n": m, "radix_passes_run": ex_passes, "auc": exact,
            "ms_median": ex_ms, "ms_min": float(np.min(ex_ev)), "ms_max": float(np.max(ex_ev)),
            "host_ms_median": float(np.median(ex_host)),
            "bytes_from_shape": int(exact_bytes),
            "GBps_from_shape": exact_bytes / (ex_ms * 1e-3) / 1e9,
            "examples_per_s": m / (ex_ms * 1e-3),
            "includes": "hipMalloc / hipFree of its buffers and two host waits",
        },
        "not_tried": ["the other merge form (resident entries appended to the batch before "
                      "the sort)", "passes that skip on a device-side word (an add with no host wait and "
                      "few passes; the eight-pass A/B is profiles/auc_ab_span_wait.txt)",
                      "kernel-level times (no profiler run)"],
        "lib": os.path.basename(_lib.LIB_PATH),
    }
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    if a.index:
        line = ("| `%s` | `tools/bench_auc.py`: one `psg_auc_add_dev` of %d examples onto %d "
                "resident keys (%.3f ms) and `psg_auc_exact_dev` over %d (%.3f ms); HIP events, "
                "medians. |\n" % (os.path.basename(a.out), n, resident_before, add_ms, m, ex_ms))
        old = open(a.index).read() if os.path.exists(a.index) else ""
        kept = [l for l in old.splitlines(True) if not l.startswith("| `%s` |" %
                                                                    os.path.basename(a.out))]
        with open(a.index, "w") as f:
            f.write("".join(kept) + ("" if not kept or kept[-1].endswith("\n") else "\n") + line)
    auc.close()
    mb.close()
    L.psg_destroy(ctx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
