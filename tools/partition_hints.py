#!/usr/bin/env python3
"""What the search partition's hints (psg_partition.hip search_item) cost
when they miss.

A cfg2-shaped plan (bench.py's headline: --batch aggregates of 8 pushes x
131,072 keys) is stepped while the keys in its push buffers are replaced
before every step, from one of two key sets staged on the device: set A (the
pushes as generated) and set B (every aggregate's pushes rotated by one, so
the same lengths and all keys in D, but other cuts).  Three cases, the copy
into the push buffers the same in all of them:

  hit   hints on,  A copied in before every step: every hint holds
  miss  hints on,  A and B alternating:           (nearly) every hint fails
  off   PSG_NO_HINTS, A and B alternating:        the plain search

Per case the partition's and the whole step's time by HIP events (as
bench.py's partition_pass), the mean over --steps alternations; the cases
are interleaved --rounds times and every round is printed, so the spread of
`off` from round to round is there to set `miss - off` against.  The share
of hints that hold from A to B is counted on the host (a hint holds iff both
sets have the same cut).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE = 1024  # cfg2: 8 pushes per job, 1024-slot tiles (psg_internal.h kTileSlots)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    from parameter_server_amd import _lib, synth
    from parameter_server_amd.kv_vector import MergePlan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream

    def to_dev(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    insts = [synth.shard_instance(seed=1 + j, lo=0, hi=(1 << 64) - 1) for j in range(args.batch)]
    jobs, keep, setA, setB, arena = [], [], [], [], []
    same = total = 0
    for D, pushes in insts:
        np_ = len(pushes)
        n = [k.size for k, _ in pushes]
        assert len(set(n)) == 1, "the rotation needs pushes of one length"
        ka = np.concatenate([k for k, _ in pushes])
        kb = np.concatenate([pushes[(p + 1) % np_][0] for p in range(np_)])
        x = D[::TILE]
        for p in range(np_):
            ca = np.searchsorted(pushes[p][0], x)
            cb = np.searchsorted(pushes[(p + 1) % np_][0], x)
            same += int(np.sum(ca == cb)) + 1  # and the end boundary: n in both
            total += x.size + 1
        dD, buf = to_dev(D), to_dev(ka)
        va = to_dev(np.concatenate([vs[0] for _, vs in pushes]))
        out = torch.empty(D.size, dtype=torch.float32, device=dev)
        offs = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        keep.append((dD, va, out))
        arena.append(buf)
        setA.append(to_dev(ka))
        setB.append(to_dev(kb))
        jobs.append({"keys": dD.data_ptr(), "nslots": int(D.size),
                     "push_keys": [buf[offs[p]:].data_ptr() for p in range(np_)],
                     "push_vals": [[va[offs[p]:].data_ptr()] for p in range(np_)],
                     "push_n": [int(v) for v in n], "out": [out.data_ptr()]})
    plans = {"on": MergePlan(0, _lib.PSG_F32, 1, jobs),
             "off": MergePlan(0, _lib.PSG_F32, 1, jobs, flags=_lib.PSG_NO_HINTS)}
    want = np.array([v for jb in jobs for v in jb["push_n"]], np.uint64)

    def fill(sets):
        for buf, src in zip(arena, sets):
            buf.copy_(src, non_blocking=True)

    def case(plan, alternate, K):
        """Mean (partition ms, step ms) over K steps, keys copied in before each."""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(K)]
        for s in range(K):
            fill(setB if alternate and s % 2 else setA)
            ev[s][0].record(stream)
            plan.run_stage(0, sh)
            ev[s][1].record(stream)
            plan.run_stage(1, sh)
            ev[s][2].record(stream)
        torch.cuda.synchronize()
        assert np.array_equal(plan.matched(), want), "unmatched keys"
        return (float(np.mean([e[0].elapsed_time(e[1]) for e in ev])),
                float(np.mean([e[0].elapsed_time(e[2]) for e in ev])))

    cases = {"hit": ("on", False), "miss": ("on", True), "off": ("off", True)}
    for name, (pl, alt) in cases.items():
        case(plans[pl], alt, args.warmup)
    rounds = {name: [] for name in cases}
    for _ in range(args.rounds):
        for name, (pl, alt) in cases.items():
            case(plans[pl], alt, 4)  # the case's own steady state (seg of its last step)
            rounds[name].append(case(plans[pl], alt, args.steps))
    res = {"tool": "partition_hints", "batch": args.batch, "steps": args.steps,
           "rounds": args.rounds, "hints_that_hold_A_to_B": same / total}
    for name, r in rounds.items():
        part, step = [x[0] for x in r], [x[1] for x in r]
        res[name] = {"partition_ms": part, "step_ms": step,
                     "partition_ms_median": float(np.median(part)),
                     "step_ms_median": float(np.median(step)),
                     "step_ms_min": min(step), "step_ms_max": max(step)}
    res["miss_minus_off_step_ms"] = res["miss"]["step_ms_median"] - res["off"]["step_ms_median"]
    res["off_step_spread_ms"] = res["off"]["step_ms_max"] - res["off"]["step_ms_min"]
    print(json.dumps(res), flush=True)
    for p in plans.values():
        p.close()


if __name__ == "__main__":
    main()
