"""MEASUREMENT AID: the device-resident Darling worker (psg_mb_darling_*).

Prints one JSON object and writes it to --out (profiles/darling_worker.json):

  init_ms        psg_mb_darling_init on a localized minibatch, which ends in a
                 device wait: the state, the stable sort of the surviving
                 pairs by row and the columns' ranges to the host;
  pass_ms        one whole data pass: psg_mb_darling_gradients and
                 psg_mb_darling_update_dual for every block in turn, all
                 enqueued, then one device wait; gradients_ms / update_dual_ms
                 are the same pass with only the one call per block;
  longest_column the entries of the longest column as a share of all, and the
                 time of psg_mb_darling_gradients over that one column as a
                 share of gradients_ms.

Host clock around enqueue + wait; every figure is the median over --steps
timed repeats after --warmup untimed ones.  The workload is tools/
bench_worker.py's minibatch (seeded, stated in the output); the dictionary is
its distinct ids cut into --blocks blocks of equally many keys.  The pulled
weights alternate between two vectors 0.01 apart, so that every pass has
delta_w != 0 on every column and dual returns to where it was.  G, U and the
weights stay on the device: the calls are the C ABI's, not
DarlingWorker.block_step's, whose host round trip is not what is measured.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_worker import minibatch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--mean-nnz", type=int, default=64)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--binary", action="store_true")
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "darling_worker.json"))
    a = ap.parse_args()

    import torch
    from parameter_server_amd import _lib
    from parameter_server_amd.worker import Minibatch

    L = _lib.lib()
    table = np.random.default_rng(a.seed).integers(0, 1 << 64, size=a.universe, dtype=np.uint64)
    offset, index, value, y = minibatch(a.seed * 1000, a.rows, a.mean_nnz, a.zipf, a.universe,
                                        table)
    dic, counts = np.unique(index, return_counts=True)
    nd, nnz = dic.size, index.size
    bounds = np.linspace(0, nd, a.blocks + 1).astype(np.int64)
    longest = int(np.argmax(counts))

    ctx = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(ctx)))
    mb = Minibatch(ctx)
    mb.load(offset, index, None if a.binary else value, y)
    mb.uniq()
    rng = np.random.default_rng(a.seed + 7)
    w = [rng.standard_normal(nd) * 0.05]
    w.append(w[0] + np.where(rng.random(nd) < 0.5, 0.01, -0.01))
    d_dic = torch.from_numpy(dic.view(np.int64)).to("cuda:0")
    d_w = [torch.from_numpy(x).to("cuda:0") for x in w]
    d_g = torch.zeros(nd, dtype=torch.float64, device="cuda:0")
    d_u = torch.zeros(nd, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    mb.localize(d_dic.data_ptr(), nd)
    wait = torch.cuda.synchronize

    def init():
        _lib.check(L.psg_mb_darling_init(mb._h, 1.0, d_w[0].data_ptr(), None))

    def gradients(cb, ce):
        _lib.check(L.psg_mb_darling_gradients(mb._h, cb, ce, d_g.data_ptr() + 8 * cb,
                                              d_u.data_ptr() + 8 * cb, None))

    def update(cb, ce, which):
        _lib.check(L.psg_mb_darling_update_dual(mb._h, cb, ce, d_w[which].data_ptr() + 8 * cb,
                                                5.0, None))

    def timed(fn, reps, warm):
        ms = []
        for i in range(warm + reps):
            wait()
            t0 = time.perf_counter()
            fn(i)
            wait()
            if i >= warm:
                ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(np.min(ms))

    blocks = [(int(bounds[b]), int(bounds[b + 1])) for b in range(a.blocks)]

    def whole(i):
        for cb, ce in blocks:
            gradients(cb, ce)
            update(cb, ce, (i + 1) % 2)

    def only_g(i):
        for cb, ce in blocks:
            gradients(cb, ce)

    def only_u(i):
        for cb, ce in blocks:
            update(cb, ce, (i + 1) % 2)

    init_ms = timed(lambda i: init(), a.steps, a.warmup)
    pass_ms = timed(whole, a.steps, a.warmup)
    g_ms = timed(only_g, a.steps, a.warmup)
    u_ms = timed(only_u, a.steps, a.warmup)
    one_ms = timed(lambda i: gradients(longest, longest + 1), a.steps, a.warmup)
    objv = C.c_double()
    _lib.check(L.psg_mb_darling_objv(mb._h, C.byref(objv), None))
    out = {
        "tool": "bench_darling_worker",
        "workload": {"rows": a.rows, "mean_nnz_per_row": a.mean_nnz, "nnz": int(nnz),
                     "zipf_exponent": a.zipf, "universe": a.universe, "ndict": int(nd),
                     "binary": bool(a.binary), "blocks": a.blocks,
                     "longest_column": int(counts.max()),
                     "median_column": float(np.median(counts)), "seed": a.seed},
        "method": {"steps": a.steps, "warmup": a.warmup,
                   "timer": "host clock around enqueue + device wait", "figure": "median"},
        "init_ms": init_ms[0], "init_ms_min": init_ms[1],
        "pass_ms": pass_ms[0], "pass_ms_min": pass_ms[1],
        "gradients_ms": g_ms[0], "gradients_ms_min": g_ms[1],
        "update_dual_ms": u_ms[0], "update_dual_ms_min": u_ms[1],
        "pairs_per_s_pass": nnz / (pass_ms[0] * 1e-3),
        "longest_column": {"entries_share": float(counts.max() / nnz),
                           "gradients_ms": one_ms[0],
                           "share_of_gradients_ms": one_ms[0] / g_ms[0]},
        "last_objv": objv.value,
        "lib": os.path.basename(_lib.LIB_PATH),
    }
    mb.close()
    L.psg_destroy(ctx)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
