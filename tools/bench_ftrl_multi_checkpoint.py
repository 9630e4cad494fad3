"""MEASUREMENT AID: checkpoint and restore of the multi-model FTRL (DESIGN.md
4.14b) against the only other ways to move that much state.

For a model of --entries keys (2^22) and every m of --models (1, 4, 8, 16, 32)
it times, with device arrays and HIP events around each whole region:

  export        psg_ftrlm_export_state_dev of the whole sweep (flag count and
                scan, device sort by key, row gather);
  export_scalar m psg_ftrl_export_state_dev calls on m scalar models that hold
                the same keys;
  import        psg_ftrlm_import_dev of that image into a reserved empty model;
  import_scalar m psg_ftrl_import_dev calls into m reserved empty scalar models;
  push          psg_ftrlm_push_dev of the same keys, all new: the same index
                walk and row write as the import.

Method as tools/bench_ftrl_checkpoint.py's: seeded inputs, one untimed run of
every region of every shape first, then --steps repetitions (at least 5) with
the regions of the two sides alternating in one process, the median reported
with min and max.  The image is imported and the keys are pushed in messages of
--msg keys.  A fresh model (init and reserve, untimed) precedes each import and
push repetition.  Not measured: the host forms, an import that has to grow the
table, a range export, and psg_ftrlm_import_weights_dev.

Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--entries", type=int, default=1 << 22)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--msg", type=int, default=1 << 20, help="keys per import / push message")
    ap.add_argument("--steps", type=int, default=5, help="repetitions of each timed region")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ftrl_multi_checkpoint.json"))
    args = ap.parse_args()
    assert args.steps >= 5, "the median of at least 5 runs"

    import torch
    from parameter_server_amd import _lib
    from parameter_server_amd.ftrl import FTRLModel, FTRLMultiModel
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    rng = np.random.default_rng(args.seed)
    keys = np.unique(rng.integers(0, 1 << 64, size=args.entries, dtype=np.uint64))
    n = keys.size
    cuts = [(lo, min(lo + args.msg, n)) for lo in range(0, n, args.msg)]
    gen = torch.Generator(device=dev).manual_seed(args.seed)

    def put(a):
        return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)).to(dev)

    def at(t, lo, width=1):
        return t.data_ptr() + t.element_size() * lo * width

    d_keys = put(keys)
    d_pos = put(rng.integers(0, 1 << 20, size=n, dtype=np.uint64))
    d_neg = put(rng.integers(0, 1 << 20, size=n, dtype=np.uint64))
    d_p32 = put(rng.integers(0, 6, size=n).astype(np.uint32))
    d_n32 = put(rng.integers(0, 6, size=n).astype(np.uint32))
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def timed(regions, before):
        """regions: name -> body; before: name -> untimed preparation (or None).
        One untimed pass, then --steps passes with the regions alternating:
        name -> event seconds of each pass."""
        sec = {name: [] for name in regions}
        for i in range(args.steps + 1):
            for name, body in regions.items():
                if before.get(name):
                    before[name]()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                body()
                b.record()
                torch.cuda.synchronize()
                if i:
                    sec[name].append(a.elapsed_time(b) * 1e-3)
        return sec

    def rate(sec):
        return {"keys_per_s": n / statistics.median(sec), "ms_median": statistics.median(sec) * 1e3,
                "ms_min": min(sec) * 1e3, "ms_max": max(sec) * 1e3}

    shapes = {}
    for m in args.models:
        params = [dict(alpha=0.1 + 0.01 * j, beta=1.0, lambda1=1.0, lambda2=0.1) for j in range(m)]
        w = torch.randn((n, m), dtype=torch.float64, device=dev, generator=gen)
        w[torch.rand((n, m), device=dev, generator=gen) < 0.5] = -0.0  # thresholded weights
        z = torch.randn((n, m), dtype=torch.float64, device=dev, generator=gen)
        grad = torch.randn((n, m), dtype=torch.float64, device=dev, generator=gen)
        w_col = [w[:, j].contiguous() for j in range(m)]
        z_col = [z[:, j].contiguous() for j in range(m)]
        out = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in ("keys", "pos", "neg")}
        out_w, out_z = torch.zeros_like(w), torch.zeros_like(z)
        col = {k: torch.zeros(n, dtype=torch.int64, device=dev)
               for k in ("keys", "pos", "neg", "w", "z")}

        multi = FTRLMultiModel(params)
        L, h = multi._L, multi._h
        parr = (_lib.FtrlParam * m)(*[_lib.FtrlParam(p["alpha"], p["beta"], p["lambda1"],
                                                     p["lambda2"]) for p in params])
        scalars = []
        for p in params:
            s = FTRLModel(0)
            s.setLearningRate(p["alpha"], p["beta"])
            s.setPenalty(p["lambda1"], p["lambda2"])
            scalars.append((s, s._model(), _lib.FtrlParam(p["alpha"], p["beta"], p["lambda1"],
                                                          p["lambda2"])))

        def fresh_multi():
            _lib.check(L.psg_ftrlm_init(h, parr, m, 0))
            _lib.check(L.psg_ftrlm_reserve(h, n))

        def fresh_scalars():
            for _, hs, ps in scalars:
                _lib.check(L.psg_ftrl_init(hs, C.byref(ps), 0))
                _lib.check(L.psg_ftrl_reserve(hs, n))

        def do_import():
            for lo, hi in cuts:
                _lib.check(L.psg_ftrlm_import_dev(h, at(d_keys, lo), hi - lo, at(d_pos, lo),
                                                  at(d_neg, lo), at(w, lo, m), at(z, lo, m),
                                                  stream))

        def do_import_scalar():
            for j, (_, hs, _) in enumerate(scalars):
                for lo, hi in cuts:
                    _lib.check(L.psg_ftrl_import_dev(hs, at(d_keys, lo), hi - lo, at(d_pos, lo),
                                                     at(d_neg, lo), at(w_col[j], lo),
                                                     at(z_col[j], lo), stream))

        def do_push():
            for lo, hi in cuts:
                _lib.check(L.psg_ftrlm_push_dev(h, at(d_keys, lo), hi - lo, at(d_p32, lo),
                                                at(d_n32, lo), at(grad, lo, m), stream))

        def do_export():
            _lib.check(L.psg_ftrlm_export_state_dev(
                h, None, out["keys"].data_ptr(), out["pos"].data_ptr(), out["neg"].data_ptr(),
                out_w.data_ptr(), out_z.data_ptr(), n, count.data_ptr(), stream))

        def do_export_scalar():
            for _, hs, _ in scalars:
                _lib.check(L.psg_ftrl_export_state_dev(
                    hs, None, col["keys"].data_ptr(), col["pos"].data_ptr(), col["neg"].data_ptr(),
                    col["w"].data_ptr(), col["z"].data_ptr(), n, count.data_ptr(), stream))

        sec = timed({"push": do_push, "import": do_import, "import_scalar": do_import_scalar},
                    {"push": fresh_multi, "import": fresh_multi, "import_scalar": fresh_scalars})
        # the last import of each side is what the exports read
        assert multi.status()[0] == n and scalars[-1][0].status()[0] == n
        sec.update(timed({"export": do_export, "export_scalar": do_export_scalar}, {}))
        assert int(count.cpu()[0]) == n
        assert torch.equal(out["keys"], d_keys) and torch.equal(out["pos"], d_pos)
        assert torch.equal(out_w.view(torch.int64), w.view(torch.int64))
        assert torch.equal(out_z.view(torch.int64), z.view(torch.int64))
        assert torch.equal(col["w"], w_col[-1].view(torch.int64))
        med = {k: statistics.median(v) for k, v in sec.items()}
        shapes[str(m)] = {
            **{k: rate(v) for k, v in sec.items()},
            "export_scalar_over_export": med["export_scalar"] / med["export"],
            "import_scalar_over_import": med["import_scalar"] / med["import"],
            "push_over_import": med["push"] / med["import"],
            "image_bytes_per_key": 24 + 16 * m,
        }
        multi.close()
        for s, _, _ in scalars:
            s.close()
        del w, z, grad, w_col, z_col, out_w, out_z
        torch.cuda.empty_cache()

    result = {
        "metric": "ftrl_multi_checkpoint", "unit": "keys/s",
        "shape": {"entries": int(n), "message_keys": args.msg, "messages": len(cuts),
                  "repetitions": args.steps, "seed": args.seed, "models": args.models},
        "gpu": shapes,
        "not_measured": ["host forms", "an import that grows the table", "a range export",
                         "psg_ftrlm_import_weights_dev"],
    }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
