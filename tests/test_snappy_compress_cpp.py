"""The snappy encoder's host twin (parameter_server_amd/csrc/psg_snappy_enc.cc
over psg_snappy_enc.h) on the edge inputs, with source and destination heap
buffers of the exact lengths and a guard behind the maximum compressed length,
as a stand-alone host program built with plain g++ under the address and
undefined-behaviour sanitizers.  It is the source file libpsg.so is built
from; the program links no HIP library and needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cpp") / "test_snappy_enc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "test_snappy_enc.cc"),
           os.path.join(ROOT, "parameter_server_amd", "csrc", "psg_snappy_enc.cc"),
           "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_snappy_encoder_edges(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
