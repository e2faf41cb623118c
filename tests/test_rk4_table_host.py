"""csrc/rk4_table.hpp on its own (the RK4 stage kinds: their arithmetic against the reference's sequence, their access flags, the touch
counts derived from the flags): tests/host/rk4_table_check.cpp, built with the host compiler (no HIP, no GPU) and run.
-ffp-contract=off: "the same operations in the same order" is then exact on the host."""

import os
import shutil
import subprocess

from conftest import ROOT


def test_rk4_table_host_program(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "rk4_table_check")
    src = os.path.join(ROOT, "tests", "host", "rk4_table_check.cpp")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RK4_TABLE_OK" in r.stdout, r.stdout + r.stderr
