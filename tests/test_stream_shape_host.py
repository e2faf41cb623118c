"""csrc/stream_shape.hpp on its own (the streaming policy, the alignment rule, the grid rule, the pieces of a launch, the tag
dispatchers): tests/host/stream_shape_check.cpp, built with the host compiler (no HIP, no GPU) and run."""

import os
import shutil
import subprocess

from conftest import ROOT


def test_stream_shape_host_program(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "stream_shape_check")
    src = os.path.join(ROOT, "tests", "host", "stream_shape_check.cpp")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "STREAM_SHAPE_OK" in r.stdout, r.stdout + r.stderr
