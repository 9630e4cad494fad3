"""MEASUREMENT AID: the device-resident FTRL model (psg_ftrl_*) at a size that
misses every cache -- 2^24 entries, messages of 131,072 uniform 64-bit keys.

Prints one JSON line: keys/s of psg_ftrl_push_dev with every key resident and
with 10 % of the keys new, keys/s of psg_ftrl_pull_dev, the cost of one rehash,
and the same update over std::unordered_map on one CPU core (tools/ftrl_cpu,
compiled on the fly, run in this process).  Method as bench.py's: seeded
inputs, --prewarm-ms of untimed messages before each timed region, HIP events
around K whole messages.

HBM bytes per key come from counters collected in runs of their own, one
counter per pass (the two do not fit one pass) and nothing traced beside them:
    for c in FETCH_SIZE WRITE_SIZE; do
      rocprofv3 --pmc $c --output-format csv -d DIR/$c -o run -- \\
          python tools/ftrl_bench.py --pmc-child --steps 8; done
    python tools/ftrl_bench.py --pmc-dir DIR --pmc-steps 8
((2 x FETCH_SIZE + WRITE_SIZE) x 1 KiB per dispatch, the gfx950 correction),
and are set against the line-granular bound: a pushed key moves 24 B of
message, reads one 128-B bucket and writes it back.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAM = dict(alpha=0.1, beta=1.0, lambda1=1.0, lambda2=0.1)
PUSH_BOUND = 8 + 4 + 4 + 8 + 128 + 128   # message + bucket read + bucket written
PULL_BOUND = 8 + 128 + 8                 # key + bucket read + weight written


def sample(rng, resident, n, new_frac):
    """A message of n strictly increasing keys: resident ones, new_frac of
    them replaced by keys never seen."""
    nnew = int(round(n * new_frac))
    idx = np.unique(rng.integers(0, resident.size, size=2 * (n - nnew)))
    idx = np.sort(rng.permutation(idx)[:n - nnew])
    keys = resident[idx]
    if nnew:
        keys = np.union1d(keys, rng.integers(0, 1 << 64, size=nnew, dtype=np.uint64))
    assert keys.size == n, "key collision: change the seed"
    return (keys, rng.integers(0, 6, size=n).astype(np.uint32),
            rng.integers(0, 6, size=n).astype(np.uint32), rng.standard_normal(n))


class Device:
    """The model and the messages on cuda:0."""

    def __init__(self, entries):
        import torch
        from parameter_server_amd import _lib
        from parameter_server_amd.ftrl import FTRLModel
        assert torch.cuda.is_available(), "this measurement needs a GPU"
        self.torch, self._lib = torch, _lib
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.m = FTRLModel(0)
        self.m.setLearningRate(PARAM["alpha"], PARAM["beta"])
        self.m.setPenalty(PARAM["lambda1"], PARAM["lambda2"])
        self.m.reserve(entries + entries // 2)
        self.L, self.h = self.m._L, self.m._h

    def put(self, msg):
        t = self.torch
        k, p, n, g = msg
        return (t.from_numpy(k.view(np.int64)).to(self.dev), t.from_numpy(p.view(np.int32)).to(self.dev),
                t.from_numpy(n.view(np.int32)).to(self.dev), t.from_numpy(g).to(self.dev))

    def push(self, d):
        self._lib.check(self.L.psg_ftrl_push_dev(self.h, d[0].data_ptr(), d[0].numel(),
                                                 d[1].data_ptr(), d[2].data_ptr(),
                                                 d[3].data_ptr(), self.stream))

    def pull(self, d, out):
        self._lib.check(self.L.psg_ftrl_pull_dev(self.h, d[0].data_ptr(), d[0].numel(),
                                                 out.data_ptr(), self.stream))

    def timed(self, calls, warm, prewarm_ms):
        """Seconds of `calls` (a list of thunks) after prewarm_ms of `warm`."""
        t = self.torch
        t.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < prewarm_ms:
            for f in warm:
                f()
            t.cuda.synchronize()
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record()
        for f in calls:
            f()
        b.record()
        t.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3


def build_inputs(args):
    rng = np.random.default_rng(args.seed)
    resident = np.unique(rng.integers(0, 1 << 64, size=args.entries, dtype=np.uint64))
    fill = []
    for lo in range(0, resident.size, 1 << 20):
        k = resident[lo:lo + (1 << 20)]
        fill.append((k, rng.integers(0, 6, size=k.size).astype(np.uint32),
                     rng.integers(0, 6, size=k.size).astype(np.uint32), rng.standard_normal(k.size)))
    res = [sample(rng, resident, args.msg, 0.0) for _ in range(args.steps)]
    new = [sample(rng, resident, args.msg, args.new_frac) for _ in range(args.steps)]
    return resident, fill, res, new


def pmc_child(args):
    """Under rocprofv3: fill, then K resident pushes, K pushes with new keys,
    K pulls -- the dispatches --pmc-dir reads, in this order."""
    resident, fill, res, new = build_inputs(args)
    D = Device(resident.size)
    for msg in fill:
        D.push(D.put(msg))
    dres, dnew = [D.put(m) for m in res], [D.put(m) for m in new]
    out = D.torch.zeros(args.msg, dtype=D.torch.float64, device=D.dev)
    for d in dres:
        D.push(d)
    for d in dnew:
        D.push(d)
    for d in dres:
        D.pull(d, out)
    D.torch.cuda.synchronize()
    D.m.close()


def pmc_read(path, steps, msg):
    """Mean HBM bytes per key of the last dispatches of each kernel.  The
    passes run the same program, so a kernel's n-th dispatch is the same
    message in each."""
    per = {}
    for f in glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r.get("Kernel_Name", "")
                kern = "update" if "ftrl_update_kernel" in name else \
                    "pull" if "ftrl_pull_kernel" in name else None
                if kern:
                    d = per.setdefault(kern, {}).setdefault(r["Counter_Name"], {})
                    i = int(r["Dispatch_Id"])
                    d[i] = d.get(i, 0.0) + float(r["Counter_Value"])
    if "update" not in per or "pull" not in per:
        return None

    def mean(kern, sl):
        def vals(counter):
            d = per[kern][counter]
            return [d[i] for i in sorted(d)][sl]
        b = [(2 * f + w) * 1024 for f, w in zip(vals("FETCH_SIZE"), vals("WRITE_SIZE"))]
        return sum(b) / len(b) / msg

    out = {"push_resident": mean("update", slice(-2 * steps, -steps)),
           "push_new": mean("update", slice(-steps, None)),
           "pull": mean("pull", slice(-steps, None))}
    return {"source": "rocprofv3 --pmc, one pass per counter: (2 x FETCH_SIZE + WRITE_SIZE) x 1 KiB",
            "bytes_per_key": out,
            "bound_bytes_per_key": {"push": PUSH_BOUND, "pull": PULL_BOUND},
            "ratio_to_bound": {"push_resident": out["push_resident"] / PUSH_BOUND,
                               "push_new": out["push_new"] / PUSH_BOUND,
                               "pull": out["pull"] / PULL_BOUND}}


def cpu_baseline(args, resident, fill, res, new):
    tmp = tempfile.mkdtemp(prefix="ftrl_cpu")
    so = os.path.join(tmp, "libftrl_cpu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                    os.path.join(ROOT, "tools", "ftrl_cpu", "ftrl_cpu.cc")], check=True)
    L = C.CDLL(so)
    L.ftrl_cpu_new.restype = C.c_void_p
    L.ftrl_cpu_new.argtypes = [C.c_double] * 4 + [C.c_size_t]
    L.ftrl_cpu_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
    L.ftrl_cpu_pull.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.ftrl_cpu_free.argtypes = [C.c_void_p]
    h = L.ftrl_cpu_new(PARAM["alpha"], PARAM["beta"], PARAM["lambda1"], PARAM["lambda2"],
                       resident.size + resident.size // 2)

    def push(m):
        L.ftrl_cpu_push(h, m[0].ctypes.data, m[0].size, m[1].ctypes.data, m[2].ctypes.data,
                        m[3].ctypes.data)

    for m in fill:
        push(m)
    k = min(args.cpu_steps, len(res))
    push(res[-1])   # untimed
    t0 = time.perf_counter()
    for m in res[:k]:
        push(m)
    t1 = time.perf_counter()
    for m in new[:k]:
        push(m)
    t2 = time.perf_counter()
    out = np.zeros(args.msg)
    for m in res[:k]:
        L.ftrl_cpu_pull(h, m[0].ctypes.data, m[0].size, out.ctypes.data)
    t3 = time.perf_counter()
    L.ftrl_cpu_free(h)
    return {"what": "std::unordered_map on one core, same model and messages, %d messages each" % k,
            "push_resident_keys_per_s": k * args.msg / (t1 - t0),
            "push_new_keys_per_s": k * args.msg / (t2 - t1),
            "pull_keys_per_s": k * args.msg / (t3 - t2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--entries", type=int, default=1 << 24)
    ap.add_argument("--msg", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=64, help="K: whole messages per timed region")
    ap.add_argument("--new-frac", type=float, default=0.1)
    ap.add_argument("--prewarm-ms", type=float, default=100.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cpu-steps", type=int, default=8)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--pmc-child", action="store_true")
    ap.add_argument("--pmc-dir", default=None)
    ap.add_argument("--pmc-steps", type=int, default=8, help="K of the --pmc-child run")
    args = ap.parse_args()
    if args.pmc_child:
        return pmc_child(args)

    resident, fill, res, new = build_inputs(args)
    D = Device(resident.size)
    t = D.torch
    for msg in fill:
        D.push(D.put(msg))
    entries0 = D.m.status()[0]
    assert entries0 == resident.size
    dres, dnew = [D.put(m) for m in res], [D.put(m) for m in new]
    out = t.zeros(args.msg, dtype=t.float64, device=D.dev)
    warm = [lambda d=d: D.push(d) for d in dres]
    sec_res = D.timed(warm, warm, args.prewarm_ms)
    sec_pull = D.timed([lambda d=d: D.pull(d, out) for d in dres],
                       [lambda d=d: D.pull(d, out) for d in dres], args.prewarm_ms)
    sec_new = D.timed([lambda d=d: D.push(d) for d in dnew], warm, args.prewarm_ms)
    entries1 = D.m.status()[0]
    assert entries1 == entries0 + args.steps * int(round(args.msg * args.new_frac))
    # one rehash of the whole model into a table twice as large (zeroing it included)
    t.cuda.synchronize()
    t0 = time.perf_counter()
    D.m.status()
    t1 = time.perf_counter()
    D.m.reserve(2 * (entries0 + entries0 // 2) + 1)
    D.m.status()
    t2 = time.perf_counter()
    assert D.m.status()[0] == entries1
    nk = args.steps * args.msg
    traffic = None
    if args.pmc_dir:
        try:
            traffic = pmc_read(args.pmc_dir, args.pmc_steps, args.msg)
        except (KeyError, ValueError, ZeroDivisionError) as e:  # an unreadable counter file
            traffic = {"error": repr(e)}
    result = {
        "metric": "ftrl_push_keys_per_s", "value": nk / sec_res, "unit": "keys/s",
        "shape": {"entries": int(entries0), "message_keys": args.msg, "messages": args.steps,
                  "new_frac": args.new_frac, "seed": args.seed,
                  "table": "128-B buckets of 3 entries, load <= 0.5"},
        "gpu": {"push_resident_keys_per_s": nk / sec_res, "push_new_keys_per_s": nk / sec_new,
                "pull_keys_per_s": nk / sec_pull,
                "push_resident_us_per_message": sec_res / args.steps * 1e6,
                "push_new_us_per_message": sec_new / args.steps * 1e6,
                "pull_us_per_message": sec_pull / args.steps * 1e6,
                "rehash_ms": ((t2 - t1) - (t1 - t0)) * 1e3,
                "rehash_entries": int(entries1)},
        "traffic": traffic,
    }
    D.m.close()
    if not args.no_cpu_baseline:
        cpu = cpu_baseline(args, resident, fill, res, new)
        result["cpu_baseline"] = cpu
        result["speedup_vs_one_core"] = {
            "push_resident": result["gpu"]["push_resident_keys_per_s"] / cpu["push_resident_keys_per_s"],
            "push_new": result["gpu"]["push_new_keys_per_s"] / cpu["push_new_keys_per_s"],
            "pull": result["gpu"]["pull_keys_per_s"] / cpu["pull_keys_per_s"]}
        assert min(result["speedup_vs_one_core"].values()) > 1.0, "the device path must win"
    print(json.dumps(result))


if __name__ == "__main__":
    main()
