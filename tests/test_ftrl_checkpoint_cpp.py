"""The checkpoint side of the C++ FTRLModel adapter
(parameter_server_amd/csrc/ftrl_model.h: exportState, importState,
readFromFile) built with plain g++ against libpsg.so, as
tests/test_ftrl_cpp_adapter.py builds its driver.  The Python side writes a
model file and the map ``read_model_text`` reads from it; the driver parses
the same file through the adapter and compares bit for bit, and on the GPU
moves one model's state into another."""
import os
import subprocess

import numpy as np
import pytest

import ftrl_ref as R
from parameter_server_amd.ftrl import read_model_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parameter_server_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(os.path.join(LIB, "libpsg.so")):
        pytest.fail("libpsg.so not built (run __graft_entry__.build())")
    exe = str(tmp_path_factory.mktemp("cpp") / "test_ftrl_checkpoint")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "cpp", "test_ftrl_checkpoint.cc"),
           "-o", exe, f"-L{LIB}", "-lpsg", f"-Wl,-rpath,{LIB}"]
    subprocess.run(cmd, check=True)
    return exe


@pytest.fixture(scope="module", params=["f64", "f32"])
def case(request, tmp_path_factory):
    """A dump of the restated model, with overriding pairs, blank lines and
    two pairs on one line appended."""
    uni, msgs = R.parity_case(seed=4, nmsg=3, n=300, universe=500)
    ref = R.VectorFTRL(**R.PARITY_PARAM)
    for m in msgs:
        ref.push(*m)
    k, _ = R.nonzero(ref, uni)
    text = R.dump_text(ref, uni)
    text += "\n\n%d\t0.125\n  %d 1e-3 %d\t-7.5\n\n0\t2.5\n18446744073709551615 -0\n" % (
        k[3], k[10], k[3])
    d = tmp_path_factory.mktemp("ckpt")
    model, expect = str(d / "model.txt"), str(d / "expect.txt")
    with open(model, "w") as f:
        f.write(text)
    real = np.float32 if request.param == "f32" else np.float64
    keys, w = read_model_text(model, real=real)
    assert keys[0] == 0 and int(keys[-1]) == (1 << 64) - 1 and w[keys == k[3]][0] == -7.5
    with open(expect, "w") as f:
        f.write("%d\n" % keys.size)
        for a, b in zip(keys.tolist(), R.bits(w).tolist()):
            f.write("%d %x\n" % (a, b))
    return [model, expect] + (["f32"] if request.param == "f32" else [])


def test_ftrl_checkpoint_cpp_parses_the_model_file(driver, case):
    r = subprocess.run([driver, "host"] + case, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_ftrl_checkpoint_cpp_gpu(driver, case):
    r = subprocess.run([driver, "gpu"] + case, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
