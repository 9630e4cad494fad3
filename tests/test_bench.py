"""bench.py's command line: a plain run carries the headline only, --full the
blocks beside it, and --dump-outputs writes the last timed step's outputs.

The GPU cases run bench.main() in this process on a small cfg2 shape (3
aggregates of 4 pushes x 4096 keys, U = 15,154 slots each: 15 tiles, so more
than one block and a ragged last tile) and check the dumped sums bit-for-bit
against the oracle's aggregate of the same seeded inputs."""
import json
import os
import sys

import numpy as np
import pytest

import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE = dict(batch=3, npush=4, n=4096)
ARGV = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-ms", "0",
        "--batch", str(SHAPE["batch"]), "--npush", str(SHAPE["npush"]), "--n", str(SHAPE["n"])]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
BESIDE = ("f64", "cfg5", "end_to_end", "rows", "cpu_baseline")


def parse(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_is_the_default(monkeypatch):
    a = parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None
    assert (a.steps, a.warmup, a.workload, a.dtype, a.batch) == (7, 2, "cfg2", "f32", 64)
    a = parse(monkeypatch, ["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"


@pytest.fixture(scope="module")
def expected():
    """The oracle's sums and matched counts of the aggregates bench.py
    generates for SHAPE on one GPU (seed 1 + j, the whole key range)."""
    from parameter_server_amd import synth
    from parameter_server_amd.kv_vector import shard_bounds
    b = shard_bounds(1)
    sums, matched = [], []
    for j in range(SHAPE["batch"]):
        D, pushes = synth.shard_instance(seed=1 + j, lo=int(b[0]), hi=int(b[1]),
                                         npush=SHAPE["npush"], n=SHAPE["n"], overlap=0.1)
        rc, _, _, out, mt = O.aggregate(D, 0, (1 << 64) - 1, pushes)
        assert rc == 0
        sums.append(out[0])
        matched.append(mt)
    return sums, np.concatenate(matched)


def run_bench(monkeypatch, capsys, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1, "bench.py prints one JSON line"
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(monkeypatch, capsys, tmp_path, expected):
    sums, matched = expected
    d = run_bench(monkeypatch, capsys, ARGV + ["--dump-outputs", str(tmp_path)])
    assert all(k in d for k in HEADLINE) and not any(k in d for k in BESIDE)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "kv-pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    kv = SHAPE["batch"] * SHAPE["npush"] * SHAPE["n"]
    assert d["config"]["kv_per_step"] == kv
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(kv / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert sorted(os.listdir(tmp_path)) == ["matched.npy", "sums.npy"]
    got = np.load(tmp_path / "sums.npy")
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), np.concatenate(sums).view(np.uint32))
    gm = np.load(tmp_path / "matched.npy")
    assert gm.dtype == np.float64 and np.array_equal(gm, matched.astype(np.float64))


@pytest.mark.gpu
def test_full_adds_what_a_plain_run_leaves_out(monkeypatch, capsys):
    """--full with the long legs switched off by their own options: the
    roofline's own runs and the f64 block are back; a plain run has neither."""
    plain = run_bench(monkeypatch, capsys, ARGV)
    r = plain["roofline"]
    assert r["kernel_ms"] > 0 and r["partition_ms"] is None and r["measured_copy_GBps"] is None
    d = run_bench(monkeypatch, capsys, ARGV + ["--full", "--no-cfg5", "--no-cpu-baseline"])
    assert d["full"] is True and all(k in d for k in HEADLINE)
    r = d["roofline"]
    assert r["kernel_ms"] > 0 and r["partition_ms"] > 0 and r["measured_copy_GBps"] > 0
    assert d["f64"]["dtype"] == "f64" and d["f64"]["ms_per_step"] > 0
    assert "cfg5" not in d and "cpu_baseline" not in d


@pytest.mark.gpu
def test_dump_larger_than_budget_is_a_fixed_sample(monkeypatch, capsys, tmp_path, expected):
    """Sums beyond DUMP_BYTES: the same seeded share of every aggregate's
    slots, in slot order, identical from run to run."""
    import bench
    sums, _ = expected
    total = sum(s.size for s in sums)
    budget = 10000  # elements; total = 45,462
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * budget)
    a, b = tmp_path / "a", tmp_path / "b"
    run_bench(monkeypatch, capsys, ARGV + ["--dump-outputs", str(a)])
    run_bench(monkeypatch, capsys, ARGV + ["--dump-outputs", str(b)])
    got = np.load(a / "sums.npy")
    assert got.tobytes() == np.load(b / "sums.npy").tobytes()
    rng = np.random.default_rng(0)
    want = []
    for s in sums:
        idx = np.sort(rng.choice(s.size, s.size * budget // total, replace=False))
        want.append(s[idx])
    want = np.concatenate(want)
    assert 0 < want.size <= budget and got.nbytes <= bench.DUMP_BYTES
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
