"""csrc/halo_layout.hpp on its own (the exchange rule, the chunk tables, the wiring of PEER arenas, flags and segments):
tests/host/halo_layout_check.cpp, built with the host compiler (no HIP, no GPU) and run."""

import os
import shutil
import subprocess

from conftest import ROOT


def test_halo_layout_host_program(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "halo_layout_check")
    src = os.path.join(ROOT, "tests", "host", "halo_layout_check.cpp")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HALO_LAYOUT_OK" in r.stdout, r.stdout + r.stderr
