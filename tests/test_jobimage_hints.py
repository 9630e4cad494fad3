"""The job-table planner's part in the hinted search partition
(parameter_server_amd/csrc/psg_jobimage.cc, JobImage::hints): a stand-alone
host program built with plain g++ under the address and undefined-behaviour
sanitizers; it links no HIP library and needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cpp") / "test_jobimage_hints")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "test_jobimage_hints.cc"),
           os.path.join(ROOT, "parameter_server_amd", "csrc", "psg_jobimage.cc"),
           "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_hinted_image_zeroes_the_searched_seg(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
