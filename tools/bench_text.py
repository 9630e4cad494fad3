"""MEASUREMENT AID: text ingest (psg_mb_load_text) against the host parse.

The workload is bench_worker's (65 536 rows x 64 entries, Zipf 1.1 ids mapped
through a table of 64-bit keys, seed 1), rendered once as ADFEA and once as
LIBSVM with 6-decimal values.  For each format, as the median of --steps runs
after --warmup untimed ones, with at least 100 ms of untimed device work
first:

  (a) host_parse_plus_load_ms  psg_text_parse_host on one thread into arrays
                               of known size, then psg_mb_load: the path
                               without the device parse
  (b) load_text_ms             psg_mb_load_text by the host clock (it ends in
                               a device wait)
  (c) parse_ms                 its kernels by HIP events (psg_mb_profile)
  (d) h2d_copy_ms              a bare host-to-device copy of the same text
                               from pageable memory: the floor of (b)
  (e) text GB/s of (b) and (c), and the share of slow tokens

Prints one JSON object.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def render(fmt, offset, index, value, y):
    out = []
    off = offset.astype(np.int64)
    for r in range(y.size):
        b, e = off[r], off[r + 1]
        if fmt == "libsvm":
            order = np.argsort(index[b:e], kind="stable")  # idx must not decrease in a line
            ks, vs = index[b:e][order].tolist(), value[b:e][order].tolist()
            out.append("%d " % y[r] + " ".join("%d:%.6f" % kv for kv in zip(ks, vs)))
        else:
            out.append("%d 1 %d " % (r, y[r] > 0) + " ".join("%d:%d" % (k, j % 32)
                                                           for j, k in enumerate(index[b:e].tolist())))
    return ("\n".join(out) + "\n").encode()


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--mean-nnz", type=int, default=64)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--universe", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch
    from bench_worker import minibatch
    from parameter_server_amd import _lib
    from parameter_server_amd.kv_vector import _ptr
    from parameter_server_amd.worker import Minibatch, text_chunk

    L = _lib.lib()
    table = np.random.default_rng(a.seed).integers(0, 1 << 64, size=a.universe, dtype=np.uint64)
    offset, index, value, y = minibatch(a.seed * 1000, a.rows, a.mean_nnz, a.zipf, a.universe,
                                        table)
    ctx = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(ctx)))
    mb = Minibatch(ctx)
    out = {"tool": "bench_text",
           "workload": {"rows": a.rows, "mean_nnz_per_row": a.mean_nnz, "nnz": int(index.size),
                        "zipf_exponent": a.zipf, "universe": a.universe, "ids": "64-bit table",
                        "seed": a.seed, "libsvm_values": "%.6f"},
           "method": {"steps": a.steps, "warmup": a.warmup, "figure": "median",
                      "untimed_first_ms": 100, "chunk_bytes": text_chunk(),
                      "host_parse": "psg_text_parse_host, one thread, one call into sized arrays",
                      "h2d": "torch uint8 tensor from pageable memory to the device + wait"},
           "formats": {}}
    for fmt in ("adfea", "libsvm"):
        text = render(fmt, offset, index, value, y)
        f = _lib.PSG_TEXT_LIBSVM if fmt == "libsvm" else _lib.PSG_TEXT_ADFEA
        nb = len(text)
        po = np.zeros(a.rows + 1, np.uint64)
        pi = np.zeros(index.size, np.uint64)
        pv = np.zeros(index.size, np.float64) if fmt == "libsvm" else None
        py = np.zeros(a.rows, np.float64)
        res = _lib.TextResult()

        def host_path():
            _lib.check(L.psg_text_parse_host(text, nb, f, a.rows, 1, _ptr(po), _ptr(pi),
                                             _ptr(pv) if pv is not None else None, _ptr(py),
                                             a.rows, index.size, C.byref(res)))
            mb.load(po, pi, pv, py)

        def host_parse_only():
            _lib.check(L.psg_text_parse_host(text, nb, f, a.rows, 1, _ptr(po), _ptr(pi),
                                             _ptr(pv) if pv is not None else None, _ptr(py),
                                             a.rows, index.size, C.byref(res)))

        parse = []

        def device_path():
            parse.append(mb.load_text(text, f, a.rows, True).parse_ms)

        host_t = torch.frombuffer(bytearray(text), dtype=torch.uint8)
        dev_t = torch.empty(nb, dtype=torch.uint8, device="cuda:0")

        def h2d():
            dev_t.copy_(host_t)
            torch.cuda.synchronize()

        # the two paths load the same arrays
        host_path()
        want = [mb.read(n) for n in ("offset", "index", "value", "y")]
        r = mb.load_text(text, f, a.rows, True)
        got = [mb.read(n) for n in ("offset", "index", "value", "y")]
        same = all(np.array_equal(g.view(np.uint64), w.view(np.uint64)) for g, w in zip(got, want))
        assert same and r.rows == a.rows and r.bad_line == -1, "the device parse differs"

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:  # untimed: clocks up
            mb.load_text(text, f, a.rows, True)
        mb.profile(True)
        b_med, b_min = median_ms(device_path, a.steps, a.warmup)
        c_med = float(np.median(parse[a.warmup:]))
        c_min = float(np.min(parse[a.warmup:]))
        mb.profile(False)
        a_med, a_min = median_ms(host_path, a.steps, a.warmup)
        p_med, _ = median_ms(host_parse_only, max(3, a.steps // 4), 1)
        d_med, d_min = median_ms(h2d, a.steps, a.warmup)
        out["formats"][fmt] = {
            "text_bytes": nb, "bytes_per_entry": nb / index.size,
            "slow_tokens": int(r.slow_tokens),
            "slow_token_share": r.slow_tokens / float(index.size + a.rows),
            "host_parse_plus_load_ms": a_med, "host_parse_plus_load_ms_min": a_min,
            "host_parse_only_ms": p_med,
            "load_text_ms": b_med, "load_text_ms_min": b_min,
            "parse_ms": c_med, "parse_ms_min": c_min,
            "h2d_copy_ms": d_med, "h2d_copy_ms_min": d_min,
            "load_text_GBps": nb / (b_med * 1e-3) / 1e9,
            "parse_GBps": nb / (c_med * 1e-3) / 1e9,
            "speedup_b_over_a": a_med / b_med,
            "parse_over_h2d": c_med / d_med,
        }
    out["lib"] = os.path.basename(_lib.LIB_PATH)
    mb.close()
    L.psg_destroy(ctx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
