"""MEASUREMENT AID: device snappy compression (psg_snappy_compress_dev,
psg_gather_compressed).

Writes one JSON object (--out, default profiles/snappy_compress.json) and
puts a line for it into the profile index (--index).  Its sections:

* ``sizes``: for every pinned case of tests/pin_cases.snappy_cases() the raw
  length, the length of libsnappy's recorded stream (the fixture) and the
  length of ours, from the host twin.  Computed on the CPU; ``--sizes-only``
  refreshes this section alone and needs no GPU.
* ``message``: one cfg2-like message, a key part of 131,072 sorted keys below
  2^40 and 16 value parts of as many f32 in eighths, in one call.
* ``export``: one part of 256 MiB (f32 in eighths), the size of a model
  export.
  For both: the device time of the call (HIP events on the stream, median of
  --reps after at least 100 ms of untimed calls), GB/s of input, the stream
  sizes, and, where libsnappy is installed, one CPU core's snappy_compress of
  the same bytes (host clock).
* ``gather``: psg_gather_compressed against psg_gather of the same build,
  alternating, for values in eighths and for incompressible values: host
  clock around each call (both end in a device wait), median / min / max.

The kernels' shares come from a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \\
      python tools/bench_snappy_compress.py --trace-workload message
and are merged into the JSON by ``--merge-trace message=CSV export=CSV``
(no GPU needed).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("snappy_enc_setup_kernel", "snappy_enc_kernel", "snappy_enc_pack_kernel")


def sizes():
    import pin_cases as P
    from parameter_server_amd import snappy
    return {name: {"raw": len(c.data), "libsnappy": len(stream),
                   "ours": len(snappy.compress_host(c.data))}
            for name, (c, stream, _) in P.snappy_recorded().items()}


def workload(name):
    """[bytes]: the parts of the named workload."""
    import pin_cases as P
    if name == "message":
        n = 131072
        keys = P.keys_below(48000, n + 64, 40)[:n]
        assert keys.size == n
        return [P.le_bytes(keys)] + [P.le_bytes(P.quantised(48100 + i, n)) for i in range(16)]
    if name == "export":
        # 16 MiB of draws, 16 times over: the encoder sees 64 KB at a time
        return [P.le_bytes(P.quantised(48200, 4 << 20)) * 16]
    raise KeyError(name)


class Launch:
    """The device buffers of one psg_snappy_compress_dev call over `parts`."""

    def __init__(self, torch, parts):
        from parameter_server_amd import _lib, snappy
        self.L, self.check = _lib.lib(), _lib.check
        self.n = len(parts)
        soff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        doff = np.concatenate([[0], np.cumsum([snappy.max_compressed_length(len(p))
                                               for p in parts])]).astype(np.int64)
        self.total = int(soff[-1])
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).cuda()
        self.dst = torch.empty(int(doff[-1]), dtype=torch.uint8, device="cuda")
        self.soff, self.doff = torch.from_numpy(soff).cuda(), torch.from_numpy(doff).cuda()
        self.clen = torch.zeros(self.n, dtype=torch.int64, device="cuda")
        self.scratch = torch.empty(self.L.psg_snappy_compress_scratch_bytes(self.total, self.n),
                                   dtype=torch.uint8, device="cuda")
        self.host_doff = doff

    def run(self):
        self.check(self.L.psg_snappy_compress_dev(
            self.src.data_ptr(), self.soff.data_ptr(), self.n, self.dst.data_ptr(),
            self.doff.data_ptr(), self.clen.data_ptr(), self.scratch.data_ptr(), None))

    def streams(self):
        lens = self.clen.cpu().tolist()
        host = self.dst.cpu().numpy()
        return [host[int(o):int(o) + ln].tobytes() for o, ln in zip(self.host_doff[:-1], lens)]


def warm(torch, fn, ms=100):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        fn()
        torch.cuda.synchronize()


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def bench_compress(torch, name, reps):
    from parameter_server_amd import snappy
    parts = workload(name)
    lc = Launch(torch, parts)
    warm(torch, lc.run)
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lc.run()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    got = lc.streams()
    # the twin on a sample: the first part and the last (the whole export is
    # one part; its twin takes a few seconds)
    for i in sorted({0, len(parts) - 1}):
        assert got[i] == snappy.compress_host(parts[i]), "device stream differs from the twin's"
    ms = spread(ev)
    out = {"parts": len(parts), "input_bytes": lc.total,
           "fragments": sum(max(1, -(-len(p) // 65536)) for p in parts),
           "stream_bytes": [len(s) for s in got], "stream_bytes_total": sum(len(s) for s in got),
           "ratio": sum(len(s) for s in got) / lc.total,
           "device_ms": ms, "input_GBps": lc.total / (ms["median"] * 1e-3) / 1e9}
    try:
        from snappy_lib import Snappy
        S = Snappy()
        S.compress(parts[0])
        cpu = []
        for _ in range(3):
            t0 = time.perf_counter()
            lib = [S.compress(p) for p in parts]
            cpu.append((time.perf_counter() - t0) * 1e3)
        out["libsnappy_one_core"] = {"version": S.version, "ms": spread(cpu),
                                     "input_GBps": lc.total / (np.median(cpu) * 1e-3) / 1e9,
                                     "stream_bytes_total": sum(len(s) for s in lib)}
    except OSError:
        out["libsnappy_one_core"] = None
    return out


def bench_gather(torch, reps, n):
    import pin_cases as P
    from parameter_server_amd import _lib
    from parameter_server_amd.kv_vector import KVVector, Message
    D = P.keys_below(48300, 2 * n + 64, 40)
    req = np.ascontiguousarray(D[::2][:n])
    out = {}
    for kind in ("f32_eighths", "f32_incompressible"):
        W = P.quantised(48301, D.size) if kind == "f32_eighths" else \
            np.frombuffer(P.random_bytes(48302, 4 * D.size), np.float32).copy()
        W[np.isnan(W)] = 0
        v = KVVector(0)
        v.setValue(Message(key=D))
        v.set_value_array(0, W)
        # the C entries on preallocated pageable buffers, as a van would call them
        cap = v._L.psg_snappy_max_compressed_length(4 * req.size)
        raw_out, comp_out = np.empty(req.size, np.float32), np.empty(cap, np.uint8)
        nb, mt = C.c_size_t(), C.c_size_t()

        def plain():
            _lib.check(v._L.psg_gather(v._h, 0, req.ctypes.data, req.size, raw_out.ctypes.data,
                                       C.byref(mt)))

        def comp():
            _lib.check(v._L.psg_gather_compressed(v._h, 0, req.ctypes.data, req.size,
                                                  comp_out.ctypes.data, cap, C.byref(nb),
                                                  C.byref(mt)))
            return nb.value

        warm(torch, plain)
        warm(torch, comp)
        tp, tc = [], []
        for _ in range(reps):  # alternating
            t0 = time.perf_counter()
            plain()
            tp.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            nbytes = comp()
            tc.append((time.perf_counter() - t0) * 1e3)
        out[kind] = {"values": int(req.size), "raw_bytes": int(4 * req.size),
                     "stream_bytes": nbytes, "psg_gather_ms": spread(tp),
                     "psg_gather_compressed_ms": spread(tc),
                     "compressed_over_plain": float(np.median(tc) / np.median(tp))}
        v.close()
    return out


def kernel_shares(path):
    """Average ns per launch of the encoder's three kernels in a rocprofv3
    kernel trace (a file, or a directory searched for *kernel_trace.csv)."""
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[0]
    dur = {k: [] for k in KERNELS}
    for row in csv.DictReader(open(path)):
        for k in KERNELS:
            name = row["Kernel_Name"]  # demangled, or mangled with a .kd suffix
            if k + "(" in name or "%d%sE" % (len(k), k) in name or name.endswith(k):
                dur[k].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    # the untimed first launches load code objects: the later half
    avg = {k: float(np.mean(v[len(v) // 2:])) / 1e3 for k, v in dur.items()}
    total = sum(avg.values())
    return {"launches_traced": len(dur[KERNELS[1]]), "avg_us": avg,
            "pack_share_of_kernel_time": avg[KERNELS[2]] / total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--gather-n", type=int, default=1 << 20)
    ap.add_argument("--sizes-only", action="store_true")
    ap.add_argument("--trace-workload", choices=("message", "export"))
    ap.add_argument("--merge-trace", nargs="+", metavar="WORKLOAD=CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snappy_compress.json"))
    ap.add_argument("--index", default=os.path.join(ROOT, "profiles", "INDEX.md"))
    a = ap.parse_args()

    out = {}
    if os.path.exists(a.out):
        out = json.load(open(a.out))
    out["tool"] = "bench_snappy_compress"
    if a.trace_workload:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_snappy_compress.py needs a GPU: a CPU run measures nothing")
        lc = Launch(torch, workload(a.trace_workload))
        warm(torch, lc.run)
        for _ in range(a.reps):
            lc.run()
        torch.cuda.synchronize()
        return
    if a.merge_trace:
        for item in a.merge_trace:
            name, path = item.split("=", 1)
            out[name]["kernels"] = kernel_shares(path)
    else:
        out["sizes"] = sizes()
        if not a.sizes_only:
            import torch
            if not torch.cuda.is_available():
                raise SystemExit("bench_snappy_compress.py needs a GPU: a CPU run measures nothing")
            out["method"] = {"compress": "HIP events around the call on the default stream",
                             "gather": "host clock around each call; the two alternate",
                             "untimed_first_ms": 100, "reps": a.reps, "figure": "median"}
            for name in ("message", "export"):
                out[name] = bench_compress(torch, name, a.reps)
            out["gather"] = bench_gather(torch, a.reps, a.gather_n)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    if a.index and "message" in out and "export" in out:
        line = ("| `%s` | `tools/bench_snappy_compress.py`: `psg_snappy_compress_dev` of a 17-part "
                "message (%.3f ms, %.1f GB/s of input) and of one 256 MiB part (%.2f ms, %.1f "
                "GB/s); `psg_gather_compressed` against `psg_gather`; the pinned cases' raw / "
                "libsnappy / our lengths. |\n"
                % (os.path.basename(a.out), out["message"]["device_ms"]["median"],
                   out["message"]["input_GBps"], out["export"]["device_ms"]["median"],
                   out["export"]["input_GBps"]))
        old = open(a.index).read() if os.path.exists(a.index) else ""
        kept = [ln for ln in old.splitlines(True)
                if not ln.startswith("| `%s` |" % os.path.basename(a.out))]
        with open(a.index, "w") as f:
            f.write("".join(kept) + ("" if not kept or kept[-1].endswith("\n") else "\n") + line)
    print(json.dumps({k: v for k, v in out.items() if k != "sizes"}))


if __name__ == "__main__":
    main()
