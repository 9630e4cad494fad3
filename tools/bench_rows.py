#!/usr/bin/env python3
"""Row-valued pushes against what the scalar plans can do for the same data.

Workload: the cfg2 keys (8 pushes x 131,072 keys, U = 956,827 server keys)
with a row of k values per key, at (f32, 16), (f32, 64) and (f64, 8).  Per
shape, one merge is timed two ways, alternating, --rounds times each:

  rows      one RowMergePlan run (psg_rows_plan_run);
  columns   ceil(k / 4) MergePlan(m = 4) runs over the same values stored
            column by column.  The transposes in and out are not timed, which
            favours this side.

Inputs rotate over more than 512 MB of distinct buffers, 100 ms of untimed
runs come first, and the time is taken from device events around >= 20 merges.
The fold is bound by HBM bandwidth, so each time is also given as the
algorithmic bytes (psg_rows_plan_bytes) over the 8 TB/s peak and over the
copy ceiling measured in the same call (tools/copybw).  The row gather is
measured the same way on 1 M requests against k psg_gather_dev calls.

Writes profiles/rows.json (--out); needs a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBPS = 8000.0
SHAPES = (("f32", 16), ("f32", 64), ("f64", 8))


def copy_ceiling(torch, stream):
    """GB/s of the hand-written copy kernel, 1 GiB -> 1 GiB, read + write."""
    L = ctypes.CDLL(os.path.join(ROOT, "tools", "copybw", "libcopybw.so"))
    L.copybw_copy.restype = ctypes.c_int
    L.copybw_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    n = 1 << 30
    src = torch.empty(n // 4, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    ms = timed(torch, stream, [lambda: L.copybw_copy(dst.data_ptr(), src.data_ptr(), n,
                                                     stream.cuda_stream)], 10)
    return 2 * n / (ms * 1e-3) / 1e9


def timed(torch, stream, steps, reps):
    """ms per call of steps[i % len(steps)] over `reps` calls (device events),
    after 100 ms of untimed calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    i = 0
    for window in (None, reps):
        e0.record(stream)
        done = 0
        while True:
            steps[i % len(steps)]()
            i, done = i + 1, done + 1
            if window is None:  # warm up: at least 100 ms and every buffer once
                e1.record(stream)
                e1.synchronize()
                if e0.elapsed_time(e1) >= 100.0 and done >= len(steps):
                    break
            elif done == window:
                break
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(xs):
    return {"min": min(xs), "max": max(xs), "median": float(np.median(xs))}


def bench_shape(torch, stream, dname, k, rounds, reps, ceiling):
    from parameter_server_amd import _lib, synth
    from parameter_server_amd.kv_vector import MergePlan, RowMergePlan
    dtype, tdt = (np.float32, torch.float32) if dname == "f32" else (np.float64, torch.float64)
    pdt = _lib.PSG_F32 if dname == "f32" else _lib.PSG_F64
    size = np.dtype(dtype).itemsize
    D, pushes = synth.overlap_pushes(seed=1, npush=8, n=131072, dtype=dtype)
    per = (sum(s.size for s, _ in pushes) + D.size) * (8 + k * size)
    ninst = max(2, -(-(512 << 20) // per) + 1)
    sh = stream.cuda_stream
    keep, row_steps, col_steps = [], [], []
    gen = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(ninst):
        dD = torch.from_numpy(D.view(np.int64)).cuda()
        dk = [torch.from_numpy(s.view(np.int64)).cuda() for s, _ in pushes]
        rows = [torch.rand((s.size, k), dtype=tdt, device="cuda", generator=gen) for s, _ in pushes]
        cols = [r.t().contiguous() for r in rows]  # the same values, column by column
        out_r = torch.empty((D.size, k), dtype=tdt, device="cuda")
        out_c = torch.empty((k, D.size), dtype=tdt, device="cuda")
        rp = RowMergePlan(0, pdt, k, [dict(
            keys=dD.data_ptr(), nslots=D.size, push_keys=[t.data_ptr() for t in dk],
            push_rows=[t.data_ptr() for t in rows], push_n=[s.size for s, _ in pushes],
            out=out_r.data_ptr())])
        cps = []
        for c0 in range(0, k, 4):
            m = min(4, k - c0)
            cps.append(MergePlan(0, pdt, m, [dict(
                keys=dD.data_ptr(), nslots=D.size, push_keys=[t.data_ptr() for t in dk],
                push_vals=[[c[c0 + i].data_ptr() for i in range(m)] for c in cols],
                push_n=[s.size for s, _ in pushes],
                out=[out_c[c0 + i].data_ptr() for i in range(m)])]))
        keep.append((dD, dk, rows, cols, out_r, out_c, rp, cps))
        row_steps.append(lambda rp=rp: rp.run(sh))
        col_steps.append(lambda cps=cps: [p.run(sh) for p in cps])
    # the two forms give the same sums
    row_steps[0](), col_steps[0]()
    torch.cuda.synchronize()
    same = bool(torch.equal(keep[0][4].t().contiguous().view(torch.uint8),
                            keep[0][5].view(torch.uint8)))
    t_rows, t_cols = [], []
    for _ in range(rounds):
        t_rows.append(timed(torch, stream, row_steps, reps))
        t_cols.append(timed(torch, stream, col_steps, reps))
    nbytes = keep[0][6].bytes
    med = float(np.median(t_rows))
    gbps = nbytes / (med * 1e-3) / 1e9
    res = {
        "dtype": dname, "k": k, "instances": ninst, "same_bits_as_columns": same,
        "rows_ms": spread(t_rows), "columns_ms": spread(t_cols),
        "columns_plans_per_merge": -(-k // 4),
        "ratio_columns_over_rows": float(np.median(t_cols)) / med,
        "ranges_overlap": not (max(t_rows) < min(t_cols) or max(t_cols) < min(t_rows)),
        "algorithmic_bytes": nbytes, "rows_gbps": gbps,
        "fraction_of_hbm_peak": gbps / HBM_PEAK_GBPS, "fraction_of_copy_ceiling": gbps / ceiling,
        "bound": "HBM bandwidth",
    }
    # ---- the row gather on 1 M requests against k scalar gathers
    L = _lib.lib()
    rng = np.random.default_rng(3)
    req = np.unique(np.concatenate([D, rng.integers(0, 1 << 63, 200000).astype(np.uint64)]))
    req = req[: 1000000]
    dD, dreq = keep[0][0], torch.from_numpy(req.view(np.int64)).cuda()
    W = torch.rand((D.size, k), dtype=tdt, device="cuda", generator=gen)
    Wc = W.t().contiguous()
    go = torch.empty((req.size, k), dtype=tdt, device="cuda")
    gc = torch.empty((k, req.size), dtype=tdt, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    g_rows = [lambda: _lib.check(L.psg_gather_rows_dev(
        pdt, k, dD.data_ptr(), D.size, W.data_ptr(), dreq.data_ptr(), req.size, go.data_ptr(),
        cnt.data_ptr(), sh))]
    g_cols = [lambda: [_lib.check(L.psg_gather_dev(
        pdt, dD.data_ptr(), D.size, Wc[c].data_ptr(), dreq.data_ptr(), req.size, gc[c].data_ptr(),
        cnt.data_ptr(), sh)) for c in range(k)]]
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(torch, stream, g_rows, reps))
        b.append(timed(torch, stream, g_cols, reps))
    res["gather"] = {"requests": int(req.size), "rows_ms": spread(a), "scalar_calls_ms": spread(b),
                     "scalar_calls": k, "ratio_scalar_over_rows": float(np.median(b) / np.median(a)),
                     "same_bits": bool(torch.equal(go.t().contiguous().view(torch.uint8),
                                                   gc.view(torch.uint8)))}
    for x in keep:
        x[6].close()
        [p.close() for p in x[7]]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rows.py needs a GPU")
    stream = torch.cuda.current_stream()
    ceiling = copy_ceiling(torch, stream)
    out = {"device": torch.cuda.get_device_name(0), "copy_ceiling_gbps": ceiling,
           "hbm_peak_gbps": HBM_PEAK_GBPS, "rounds": args.rounds, "merges_per_timing": args.reps,
           "workload": "cfg2 keys: 8 pushes x 131,072 keys, U = 956,827", "shapes": []}
    for dname, k in SHAPES:
        out["shapes"].append(bench_shape(torch, stream, dname, k, args.rounds, args.reps, ceiling))
        print(json.dumps(out["shapes"][-1]), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
