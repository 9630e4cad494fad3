"""The C++ FTRLModel adapter (parameter_server_amd/csrc/ftrl_model.h) built
with plain g++ against libpsg.so, the way a reference server would link it
(INTEGRATION.md).  The Python side writes three messages and what the
restatement (tests/ftrl_ref.py) says a pull, nnz and the dump must be; the
driver sends them through the adapter and compares bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import ftrl_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parameter_server_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(os.path.join(LIB, "libpsg.so")):
        pytest.fail("libpsg.so not built (run __graft_entry__.build())")
    exe = str(tmp_path_factory.mktemp("cpp") / "test_ftrl_model")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "cpp", "test_ftrl_model.cc"),
           "-o", exe, f"-L{LIB}", "-lpsg", f"-Wl,-rpath,{LIB}"]
    subprocess.run(cmd, check=True)
    return exe


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    uni, msgs = R.parity_case(seed=2, nmsg=3, n=400, universe=700)
    ref = R.VectorFTRL(**R.PARITY_PARAM)
    for m in msgs:
        ref.push(*m)
    keys = np.concatenate([uni[::-1], R.absent_keys(uni, 50)])   # unsorted, some absent
    w = R.pull(ref, keys)
    dump = R.dump_text(ref, uni)
    path = str(tmp_path_factory.mktemp("ftrl") / "case.txt")
    p = R.PARITY_PARAM
    with open(path, "w") as f:
        f.write("P %s\n" % " ".join("%x" % b for b in R.bits(
            [p["alpha"], p["beta"], p["lambda1"], p["lambda2"]]).tolist()))
        for k, pos, neg, g in msgs:
            f.write("M %d\n" % k.size)
            for a, b, c, d in zip(k.tolist(), pos.tolist(), neg.tolist(), R.bits(g).tolist()):
                f.write("%d %d %d %x\n" % (a, b, c, d))
        f.write("G %d\n" % keys.size)
        for a, b in zip(keys.tolist(), R.bits(w).tolist()):
            f.write("%d %x\n" % (a, b))
        f.write("S %d\n" % ref.nnz)
        f.write("D %d\n%s" % (dump.count("\n"), dump))
    return path


def test_ftrl_cpp_adapter_builds_and_reads_the_case(driver, case):
    r = subprocess.run([driver, "host", case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_ftrl_cpp_adapter_gpu(driver, case):
    r = subprocess.run([driver, "gpu", case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
