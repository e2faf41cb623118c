"""include/fus_gpu.hpp through the compiler (no GPU, no library): tests/host/fus_gpu_hpp_check.cpp instantiates every functor class for
double and float (and P = 1 ... 10), so every typed forward is checked against its prototype in include/fus_gpu.h.  hipcc, host pass only."""

import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_every_functor_of_fus_gpu_hpp_compiles_in_both_types(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "tests", "host", "fus_gpu_hpp_check.cpp")
    b = subprocess.run([hipcc, "--cuda-host-only", "-c", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(tmp_path / "check.o"), src],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
