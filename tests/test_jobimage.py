"""The job-table planner (parameter_server_amd/csrc/psg_jobimage.cc: kernel
form, counts, image layout, shape key, fill) as a stand-alone host program
built with plain g++ under the address and undefined-behaviour sanitizers.
It is the source file libpsg.so is built from; it links no HIP library and
needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cpp") / "test_jobimage")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "test_jobimage.cc"),
           os.path.join(ROOT, "parameter_server_amd", "csrc", "psg_jobimage.cc"),
           "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_jobimage(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
