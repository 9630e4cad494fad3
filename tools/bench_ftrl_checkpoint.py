"""MEASUREMENT AID: checkpoint and restore of the device-resident FTRL model
at a size that misses every cache -- 2^24 entries.

Prints one JSON line (and writes it to --out): keys/s of
psg_ftrl_export_state_dev of the whole model (scan, device sort by key,
gather), keys/s of psg_ftrl_import_dev of that image into a reserved empty
table and into an unreserved one (the rehashes on the way included), and, as
the yardstick in the same run, keys/s of psg_ftrl_push_dev with every key new
(what tools/ftrl_bench.py measures with 10 % new keys).  Per key an import
moves 40 B of message and reads and writes one 128-B bucket, about what a push
moves (24 B of message), so its rate is expected near the push's.

Method as tools/ftrl_bench.py's: seeded inputs, one untimed run of each timed
region first (prewarm: allocations, code objects), HIP events around each
whole region, --steps repetitions, the median reported with the spread.  The
image is imported and the keys are pushed in messages of --msg keys, the same
cut for both.  A fresh model (psg_ftrl_init, untimed) precedes each
repetition.  The unreserved import waits on the host when the table has to
grow; its wall time is reported next to its event time.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAM = dict(alpha=0.1, beta=1.0, lambda1=1.0, lambda2=0.1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--entries", type=int, default=1 << 24)
    ap.add_argument("--msg", type=int, default=1 << 20, help="keys per import / push message")
    ap.add_argument("--steps", type=int, default=5, help="repetitions of each timed region")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()

    import torch
    from parameter_server_amd import _lib
    from parameter_server_amd.ftrl import FTRLModel
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    rng = np.random.default_rng(args.seed)
    keys = np.unique(rng.integers(0, 1 << 64, size=args.entries, dtype=np.uint64))
    n = keys.size
    w = rng.standard_normal(n)
    w[rng.random(n) < 0.5] = -0.0          # a trained model's share of thresholded weights
    host = dict(keys=keys, pos=rng.integers(0, 1 << 20, size=n, dtype=np.uint64),
                neg=rng.integers(0, 1 << 20, size=n, dtype=np.uint64), w=w,
                z=rng.standard_normal(n), p32=rng.integers(0, 6, size=n).astype(np.uint32),
                n32=rng.integers(0, 6, size=n).astype(np.uint32), grad=rng.standard_normal(n))

    def put(a):
        return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).to(dev)

    d = {k: put(v) for k, v in host.items()}
    out = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in ("keys", "pos", "neg", "w", "z")}
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    cuts = [(lo, min(lo + args.msg, n)) for lo in range(0, n, args.msg)]

    m = FTRLModel(0)
    m.setLearningRate(PARAM["alpha"], PARAM["beta"])
    m.setPenalty(PARAM["lambda1"], PARAM["lambda2"])
    L, h = m._L, m._model()
    param = _lib.FtrlParam(PARAM["alpha"], PARAM["beta"], PARAM["lambda1"], PARAM["lambda2"])

    def fresh(reserve):
        _lib.check(L.psg_ftrl_init(h, C.byref(param), 0))
        if reserve:
            _lib.check(L.psg_ftrl_reserve(h, n))
        torch.cuda.synchronize()

    def at(t, lo):
        return t.data_ptr() + t.element_size() * lo

    def do_import():
        for lo, hi in cuts:
            _lib.check(L.psg_ftrl_import_dev(h, at(d["keys"], lo), hi - lo, at(d["pos"], lo),
                                             at(d["neg"], lo), at(d["w"], lo), at(d["z"], lo),
                                             stream))

    def do_push():
        for lo, hi in cuts:
            _lib.check(L.psg_ftrl_push_dev(h, at(d["keys"], lo), hi - lo, at(d["p32"], lo),
                                           at(d["n32"], lo), at(d["grad"], lo), stream))

    def do_export():
        _lib.check(L.psg_ftrl_export_state_dev(h, None, out["keys"].data_ptr(),
                                               out["pos"].data_ptr(), out["neg"].data_ptr(),
                                               out["w"].data_ptr(), out["z"].data_ptr(), n,
                                               count.data_ptr(), stream))

    def timed(body, before=None):
        """(event seconds, wall seconds) of each of --steps runs after one untimed run."""
        ev, wall = [], []
        for i in range(args.steps + 1):
            if before:
                before()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            body()
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i:
                ev.append(a.elapsed_time(b) * 1e-3)
                wall.append(t1 - t0)
        return ev, wall

    def rate(sec):
        return {"keys_per_s": n / statistics.median(sec), "ms_median": statistics.median(sec) * 1e3,
                "ms_min": min(sec) * 1e3, "ms_max": max(sec) * 1e3}

    push_ev, _ = timed(do_push, lambda: fresh(True))
    assert m.status()[0] == n
    imp_ev, _ = timed(do_import, lambda: fresh(True))
    assert m.status()[:2] == (n, int(np.count_nonzero(w)))
    exp_ev, exp_wall = timed(do_export)
    assert int(count.cpu()[0]) == n
    assert np.array_equal(out["keys"].cpu().numpy().view(np.uint64), keys)
    assert np.array_equal(out["z"].cpu().numpy().view(np.uint64), host["z"].view(np.uint64))
    grow_ev, grow_wall = timed(do_import, lambda: fresh(False))
    assert m.status()[0] == n

    result = {
        "metric": "ftrl_import_keys_per_s", "value": n / statistics.median(imp_ev),
        "unit": "keys/s",
        "shape": {"entries": int(n), "message_keys": args.msg, "messages": len(cuts),
                  "repetitions": args.steps, "seed": args.seed,
                  "table": "128-B buckets of 3 entries, load <= 0.5"},
        "gpu": {"push_all_new": rate(push_ev), "import_reserved": rate(imp_ev),
                "import_unreserved": dict(rate(grow_ev),
                                          wall_ms_median=statistics.median(grow_wall) * 1e3),
                "export_state": dict(rate(exp_ev),
                                     wall_ms_median=statistics.median(exp_wall) * 1e3)},
        "import_to_push_ratio": statistics.median(push_ev) / statistics.median(imp_ev),
        "bytes_per_key_bound": {"import": 40 + 128 + 128, "push": 24 + 128 + 128},
    }
    m.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
