"""MEASUREMENT AID: one Darling data pass end to end, host form against device
form (DarlingWorker.block_step's path against darling.darling_pass).

Prints one JSON object and writes it to --out (profiles/darling_pass.json).
For each shape, on the same box in the same run, the time of one whole pass
over the key blocks -- every worker's computeGradients and push, the server's
updateWeight, every worker's pull and updateDual, block after block:

  host_*  the host form as the parent of the device forms ran it: G and U
          copied to the host and pushed by psg_push, psg_darling_update (which
          waits to read the block's violation), psg_gather to the host, the
          weights uploaded again for psg_mb_darling_update_dual -- with one
          worker this is DarlingWorker.block_step itself, with several the
          same calls in darling_pass's order (all push, one update, all pull);
  dev_*   darling_pass: psg_push_dev, psg_darling_update_dev, psg_pull_dev,
          everything enqueued, one device wait at the end of the pass.

Shapes:
  cfg1     SURVEY cfg1's stand-in for rcv1: 47,236 keys in [1, 47237), 297
           blocks, 2 workers of 10,121 rows each, f64;
  default  tools/bench_darling_worker.py's default shape: 65,536 rows, mean
           nnz 64, the dictionary cut into 16 blocks, one worker.

Host clock around enqueue + device wait; the figure is the median over --steps
timed passes after --warmup untimed ones, the two forms taking turns.  The KKT
threshold is out of reach, so no column is deactivated and every pass does the
same work.  Each shape runs in a child process of its own under `timeout -k
10`; a child that fails ends the run (nothing more is started on the device).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KMAX = (1 << 64) - 1
SHAPES = {
    "cfg1": dict(rows=20242, mean_nnz=74, zipf=1.1, universe=47236, blocks=297, workers=2,
                 hashed=False),
    "default": dict(rows=65536, mean_nnz=64, zipf=1.1, universe=1 << 22, blocks=16, workers=1,
                    hashed=True),
}
PARAM = {"eta": 1.0, "lambda_": 0.01, "kkt_filter_threshold": 1e20}
DELTA_INIT, DELTA_MAX = 1.0, 5.0


def child(name, steps, warmup, seed):
    import ctypes as C

    import torch
    from bench_worker import minibatch
    from parameter_server_amd import DarlingWorker, _lib
    from parameter_server_amd.darling import darling_pass, pass_schedule, server_progress
    from parameter_server_amd.kv_vector import KVVector, Message

    sh = SHAPES[name]
    W = sh["workers"]
    table = None
    if sh["hashed"]:
        table = np.random.default_rng(seed).integers(0, 1 << 64, size=sh["universe"],
                                                     dtype=np.uint64)
    data = []
    for w in range(W):
        offset, index, value, y = minibatch(seed * 1000 + w, sh["rows"] // W, sh["mean_nnz"],
                                            sh["zipf"], sh["universe"], table)
        if table is None:
            index = index + np.uint64(1)  # keys in [1, universe + 1)
        data.append((offset, index, value, y, np.unique(index)))
    if table is None:
        keys = np.arange(1, sh["universe"] + 1, dtype=np.uint64)
    else:
        keys = np.unique(np.concatenate([d[4] for d in data]))
    cut = np.linspace(0, keys.size, sh["blocks"] + 1).astype(np.int64)
    blocks = [(int(keys[cut[b]]), int(keys[cut[b + 1]]) if cut[b + 1] < keys.size else KMAX)
              for b in range(sh["blocks"])]

    def make():
        v = KVVector(0, _lib.PSG_F64)
        v.setValue(Message(key=keys))
        v.set_value_array(0, np.zeros(keys.size))
        _lib.check(v._L.psg_darling_init(v._h, 0, DELTA_INIT))
        ws = []
        for offset, index, value, y, dic in data:
            w = DarlingWorker(v._h, DELTA_INIT, DELTA_MAX)
            w.load(offset, index, value, y, dic)
            ws.append(w)
        return v, ws

    sched = pass_schedule([d[4] for d in data], blocks)
    nblocks = sum(1 for r in sched if r)
    p = _lib.DarlingParam(PARAM["eta"], PARAM["lambda_"], PARAM["kkt_filter_threshold"],
                          DELTA_MAX)

    def host_pass(v, ws, t):
        for (kb, ke), row in zip(blocks, sched):
            if not row:
                continue
            if W == 1:
                (i, cb, ce), = row
                ws[i].block_step(v, 0, t, cb, ce, PARAM, key_range=(kb, ke))
            else:
                for i, cb, ce in row:
                    G, U = ws[i].gradients(cb, ce)
                    v.setValue(Message(time=t, key_range=(kb, ke), key=ws[i].dict_keys[cb:ce],
                                       value=[G, U]))
                vio = C.c_double()
                _lib.check(v._L.psg_darling_update(v._h, 0, t, C.cast(C.byref(p), C.c_void_p),
                                                   C.byref(vio)))
                for i, cb, ce in row:
                    msg = Message(key=ws[i].dict_keys[cb:ce])
                    v.getValue(msg)
                    ws[i].update_dual(cb, ce, msg.value[0])
            t += 3
        return t

    def dev_pass(v, ws, t):
        return darling_pass(v, ws, 0, t, blocks, PARAM)

    forms = {"host": (host_pass,) + make(), "dev": (dev_pass,) + make()}
    ms = {"host": [], "dev": []}
    t = {"host": 0, "dev": 0}
    for step in range(warmup + steps):
        for form, (fn, v, ws) in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t[form] = fn(v, ws, t[form])
            torch.cuda.synchronize()
            if step >= warmup:
                ms[form].append((time.perf_counter() - t0) * 1e3)
    # both forms walked the same passes: the models agree bit for bit
    same = bool(np.array_equal(forms["host"][1].value(0).view(np.uint64),
                               forms["dev"][1].value(0).view(np.uint64)))
    prog = server_progress(forms["dev"][1], 0, PARAM["lambda_"])
    out = {"shape": name, "workers": W, "server_keys": int(keys.size), "blocks": nblocks,
           "rows": sh["rows"], "nnz": int(sum(d[1].size for d in data)),
           "ndict": [int(d[4].size) for d in data], "passes_timed": steps,
           "models_equal": same, "nnz_w": prog["nnz_w"]}
    for form in ("host", "dev"):
        med = float(np.median(ms[form]))
        out[form + "_ms_per_pass"] = med
        out[form + "_ms_per_pass_min"] = float(np.min(ms[form]))
        out[form + "_ms_per_block"] = med / nblocks
    out["host_over_dev"] = out["host_ms_per_pass"] / out["dev_ms_per_pass"]
    out["box"] = "%s (%s)" % (torch.cuda.get_device_name(0),
                              torch.cuda.get_device_properties(0).gcnArchName)
    for fn, v, ws in forms.values():
        for w in ws:
            w.close()
        v.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--shapes", default="cfg1,default")
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "darling_pass.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup, a.seed)
    shapes = []
    for name in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
               "--child", name, "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--seed", str(a.seed)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit("shape %s: exit status %d; nothing more is run" % (name, r.returncode))
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {
        "tool": "bench_darling_pass",
        "box": shapes[0]["box"] if shapes else None,
        "method": {"steps": a.steps, "warmup": a.warmup, "seed": a.seed,
                   "timer": "host clock around one pass: enqueue + device wait",
                   "figure": "median", "param": PARAM},
        "shapes": shapes,
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
