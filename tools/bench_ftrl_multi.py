"""MEASUREMENT AID: m FTRL models in one pass against m scalar passes.

For m in --models, on one seeded minibatch of tools/bench_worker.py's default
shape and one message of --message keys into a model of --entries entries
(DESIGN.md 4.7's sizes), this times

  times, logit, trans_times   psg_mb_gradient_rows' stages against the sum of
                              the same stages of m psg_mb_gradient calls
                              (the library's own HIP events, psg_mb_profile);
  push, pull                  psg_ftrlm_push_dev / psg_ftrlm_pull_dev against
                              m psg_ftrl_push_dev / psg_ftrl_pull_dev calls
                              (HIP events on the context's stream);
  step                        FTRLMultiWorker.step against m FTRLWorker.step
                              calls on the same minibatch (host clock; a step
                              ends in a device wait and includes the load).

The two forms alternate inside one process, --repeats times after --warmup
untimed rounds; each figure is the median with the smallest and largest
repeat beside it.  ratio = row form / (m scalar runs): below 1 the row form
wins.  Writes one JSON object to --out (default profiles/ftrl_multi.json) and
prints it.  The message's keys are all present in the model (the steady
state of a long run); the models are filled through the device forms with
room for twice --entries, so no timed push grows a table.  psg_ftrl_status /
psg_ftrlm_status run after the fill and before every round, outside the timed
regions: a rejected message fails the run, the entry counts must be --entries,
and the host's bound on the count is reset, so no timed push reads it back.
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

STAGES = ("times", "logit", "trans_times")
KEY_STEP = 0x5E3779B97  # odd, 35 bits: keys i * KEY_STEP ascend with i < 2^28 below 2^63


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def compare(rows_ms, scalar_ms):
    r, s = spread(rows_ms), spread(scalar_ms)
    return dict(rows_ms=r, scalar_x_m_ms=s, ratio=r["median"] / s["median"])


class Events:
    """A pair of HIP timing events on a given stream."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time(self, stream, work) -> float:
        assert self.hip.hipEventRecord(self.e[0], stream) == 0
        work()
        assert self.hip.hipEventRecord(self.e[1], stream) == 0
        assert self.hip.hipEventSynchronize(self.e[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e[0], self.e[1]) == 0
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="1,4,8,16,32")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--mean-nnz", type=int, default=64)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--message", type=int, default=131072)
    ap.add_argument("--entries", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sum-order", default="reference",
                    help="reference, blocked, or a comma list of worker rounds measured one after "
                         "the other (an A/B: reference,blocked,reference,blocked); both the row "
                         "and the scalar worker take the round's order")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ftrl_multi.json"))
    a = ap.parse_args()

    import torch
    from bench_worker import PARAM, minibatch
    from parameter_server_amd import _lib
    from parameter_server_amd.ftrl import FTRLModel, FTRLMultiModel
    from parameter_server_amd.worker import FTRLMultiWorker, FTRLWorker

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    L = _lib.lib()
    ev = Events()
    table = np.random.default_rng(a.seed).integers(0, 1 << 64, size=a.universe, dtype=np.uint64)
    batch = minibatch(a.seed * 1000, a.rows, a.mean_nnz, a.zipf, a.universe, table)
    assert a.entries % a.message == 0 and (a.entries - 1) * KEY_STEP < 1 << 63
    pace = a.entries // a.message
    u64 = lambda t: t.view(torch.uint8)  # noqa: E731  (bytes: torch has no uint64 arithmetic)
    all_keys = torch.arange(a.entries, dtype=torch.int64, device="cuda:0") * KEY_STEP
    msg_keys = all_keys[::pace].contiguous()  # ascending, every one present
    counts = torch.ones(a.message, dtype=torch.int32, device="cuda:0")
    rounds = a.warmup + a.repeats
    out = dict(rows=a.rows, mean_nnz=a.mean_nnz, zipf=a.zipf, universe=a.universe,
               message_keys=a.message, model_entries=a.entries, repeats=a.repeats,
               warmup=a.warmup, device=torch.cuda.get_device_name(0), models={})

    def scalar_model(hint):
        mod = FTRLModel(0, capacity_hint=hint)
        mod.setLearningRate(PARAM["alpha"], PARAM["beta"])
        mod.setPenalty(PARAM["lambda1"], PARAM["lambda2"])
        return mod

    def fill(push, grad):
        for c in range(pace):
            k = all_keys[c * a.message:(c + 1) * a.message]
            _lib.check(push(u64(k).data_ptr(), a.message, counts.data_ptr(), counts.data_ptr(),
                            grad.data_ptr()))
        torch.cuda.synchronize()

    def settled(*models):
        """status() raises on a rejected message; every key must be there"""
        for mod in models:
            entries = mod.status()[0]
            assert entries == a.entries, "%d entries, not %d" % (entries, a.entries)

    # the scalar server model and worker: one of each serves every m
    smodel = scalar_model(2 * a.entries)
    sctx = smodel._model()
    sgrad = torch.randn(a.message, dtype=torch.float64, device="cuda:0")
    fill(lambda *args: L.psg_ftrl_push_dev(sctx, *args, None), sgrad)
    sout = torch.zeros(a.message, dtype=torch.float64, device="cuda:0")
    wmodel = scalar_model(a.universe)
    sworker = FTRLWorker(wmodel)

    for m in [int(x) for x in a.models.split(",")]:
        params = [dict(PARAM, lambda1=PARAM["lambda1"] * (1 + j)) for j in range(m)]
        res = {}
        # -- server: push and pull of one message ---------------------------
        model = FTRLMultiModel(params, capacity_hint=2 * a.entries)
        ctx = model._model()
        grad = torch.randn(a.message * m, dtype=torch.float64, device="cuda:0")
        pulled = torch.zeros(a.message * m, dtype=torch.float64, device="cuda:0")
        fill(lambda *args: L.psg_ftrlm_push_dev(ctx, *args, None), grad)
        kp, cp = u64(msg_keys).data_ptr(), counts.data_ptr()
        t = {k: ([], []) for k in ("push", "pull")}
        for r in range(rounds):
            settled(model, smodel)
            got = (
                ev.time(None, lambda: _lib.check(L.psg_ftrlm_push_dev(
                    ctx, kp, a.message, cp, cp, grad.data_ptr(), None))),
                ev.time(None, lambda: [_lib.check(L.psg_ftrl_push_dev(
                    sctx, kp, a.message, cp, cp, sgrad.data_ptr(), None)) for _ in range(m)]),
                ev.time(None, lambda: _lib.check(L.psg_ftrlm_pull_dev(
                    ctx, kp, a.message, pulled.data_ptr(), None))),
                ev.time(None, lambda: [_lib.check(L.psg_ftrl_pull_dev(
                    sctx, kp, a.message, sout.data_ptr(), None)) for _ in range(m)]))
            if r >= a.warmup:
                for (rows_ms, scalar_ms), x, y in zip(t.values(), got[0::2], got[1::2]):
                    rows_ms.append(x)
                    scalar_ms.append(y)
        settled(model, smodel)
        for k, (rows_ms, scalar_ms) in t.items():
            res[k] = compare(rows_ms, scalar_ms)
        model.close()
        del grad, pulled
        # -- worker: the three stages on the resident minibatch ----------------
        wmulti = FTRLMultiModel(params, capacity_hint=a.universe)
        worker = FTRLMultiWorker(wmulti)
        mb = worker.mb
        mb.load(*batch)
        ndict = mb.uniq()
        mb.localize(mb.uniq_key_dev, ndict)
        w = torch.randn(ndict * m, dtype=torch.float64, device="cuda:0") * 0.01
        w_cols = w.view(ndict, m).t().contiguous()  # column j alone, for the scalar calls
        torch.cuda.synchronize()
        orders = a.sum_order.split(",")
        for order in orders:
            mb.set_sum_order(order)
            sworker.mb.set_sum_order(order)
            wres = {"sum_order": order}
            mb.profile(True)
            t = {s: ([], []) for s in STAGES}
            for r in range(rounds):
                mb.gradient_rows(w.data_ptr(), m)
                rows_ms = mb.stage_ms()
                scalar_ms = dict.fromkeys(STAGES, 0.0)
                for j in range(m):
                    mb.gradient(w_cols.data_ptr() + 8 * ndict * j)
                    ms = mb.stage_ms()
                    for s in STAGES:
                        scalar_ms[s] += ms[s]
                if r >= a.warmup:
                    for s in STAGES:
                        t[s][0].append(rows_ms[s])
                        t[s][1].append(scalar_ms[s])
            mb.profile(False)
            for s, (rows_ms, scalar_ms) in t.items():
                wres[s] = compare(rows_ms, scalar_ms)
            # -- the whole step, host clock -----------------------------------------
            rows_ms, scalar_ms = [], []
            for r in range(rounds):
                t0 = time.perf_counter()
                worker.step(*batch)
                t1 = time.perf_counter()
                for _ in range(m):
                    sworker.step(*batch)
                t2 = time.perf_counter()
                if r >= a.warmup:
                    rows_ms.append((t1 - t0) * 1e3)
                    scalar_ms.append((t2 - t1) * 1e3)
            wres["step"] = compare(rows_ms, scalar_ms)
            if order is orders[0]:
                res.update(wres)
            if len(orders) > 1:
                res.setdefault("rounds", []).append(wres)
        res["ndict"] = int(ndict)
        worker.close()
        wmulti.close()
        out["models"][str(m)] = res
        print("m=%d: %s" % (m, {k: round(v["ratio"], 3) for k, v in res.items()
                                if isinstance(v, dict)}), file=sys.stderr, flush=True)
    sworker.close()
    wmodel.close()
    smodel.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
