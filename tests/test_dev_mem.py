"""dev_pool (csrc/dev_mem.h), the owner of every device allocation, on the host: the stand-alone
program tests/host/dev_mem_test.cpp runs it over a malloc backend that fails each of its calls in
turn and poisons what it frees.  No GPU, nothing from HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_pool_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) on PATH")
    exe = str(tmp_path / "dev_mem_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gemma.ggml_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "dev_mem_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dev_mem_test: ok" in r.stdout
