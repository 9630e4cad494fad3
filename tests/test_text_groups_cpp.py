"""The grouped host parse (psg_text_parse_groups_host, psg_text.cc) and its
shared pieces in parameter_server_amd/csrc/psg_text.h on heap buffers with no
slack byte, as a stand-alone host program built with plain g++ under the
address and undefined-behaviour sanitizers.  They are the source files
libpsg.so is built from; the program links no HIP library and needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cpp") / "test_text_groups")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "test_text_groups.cc"),
           os.path.join(ROOT, "parameter_server_amd", "csrc", "psg_text.cc"),
           "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_grouped_parse_on_exact_buffers(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
