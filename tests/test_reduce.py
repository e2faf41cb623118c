"""The reduction entry points without a GPU: the header and its binding, the build lists, the resource pins of every shipped build of
csrc/reduce.hpp, and the launch-shape model (tests/reduce_model.py) against the header text it mirrors."""
import ctypes as C
import os
import re
import shutil

import pytest
import reduce_model as rm
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fus_gpu_reduce.h")
ENTRY_POINTS = ("fus_reduce_workspace_bytes", "fus_reduce_terms_f64", "fus_reduce_terms_f32")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_parsed_into_the_open_tier():
    lib_mod = pkg("_lib")
    assert HEADER in lib_mod.LATER_HEADER_PATHS
    functions, defines = lib_mod.parse_header(read(HEADER))
    assert tuple(functions) == ENTRY_POINTS and not defines  # no macro of its own: FUS_ABI_VERSION is fus_gpu.h's
    ptr, i64 = C.c_void_p, C.c_int64
    assert lib_mod.LATER["fus_reduce_workspace_bytes"] == (i64, [i64])
    for suf in ("f64", "f32"):
        assert lib_mod.LATER[f"fus_reduce_terms_{suf}"] == (C.c_int, [ptr] * 7 + [i64, ptr, ptr, ptr])
    assert lib_mod.ABI_VERSION == 3
    for name in ENTRY_POINTS:
        assert name not in lib_mod.DECLARATIONS and name not in lib_mod.EXTENSIONS and name not in lib_mod.ADDITIONS
    assert '#include "fus_gpu_reduce.h"' in read(ROOT, "include", "fus_gpu.hpp")


def test_library_exports_the_entry_points():
    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        assert fn.argtypes == lib_mod.LATER[name][1] and fn.restype is lib_mod.LATER[name][0]
    assert lib.fus_abi_version() == 3
    # host-only: the workspace size is the model's, and a negative n is refused
    for n in (0, 1, 255, 256, 257, 4099, rm.GRID_CAP * rm.BLOCK + 1, rm.LAUNCH_DOFS, rm.LAUNCH_DOFS + 1000, 3 * rm.LAUNCH_DOFS + 5):
        assert lib.fus_reduce_workspace_bytes(n) == rm.workspace_bytes(n), n
    assert lib.fus_reduce_workspace_bytes(-1) == -1


def test_argument_checks_launch_nothing():
    """Invalid arguments come back as FUS_ERR_INVALID_ARGUMENT before any device work: the pointers are never dereferenced (this runs
    without a GPU)."""
    lib = pkg("_lib").load()
    z, p = C.c_void_p(0), C.c_void_p(4096)
    for suf in ("f64", "f32"):
        fn = getattr(lib, f"fus_reduce_terms_{suf}")

        def call(a0=p, b0=p, c0=z, a1=z, b1=z, c1=z, x=z, n=8, out=p, ws=p):
            return fn(a0, b0, c0, a1, b1, c1, x, n, out, ws, z)

        assert call(n=-1) == -1
        assert call(out=z) == -1 and call(ws=z) == -1
        assert call(b0=z) == -1 and call(a1=p, b1=z) == -1
        assert call(out=C.c_void_p(4100)) == -1 and call(ws=C.c_void_p(4100)) == -1


def test_build_lists():
    mk = read(CSRC, "Makefile")
    src = re.search(r"^SRC = (.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR = (.*)$", mk, re.M).group(1).split()
    obj = re.search(r"^OBJ = (.*)$", mk, re.M).group(1).split()
    assert "abi_reduce.hip" in src and "_obj/abi_reduce.o" in obj
    assert "reduce.hpp" in hdr and "../../include/fus_gpu_reduce.h" in hdr  # the source hash covers them
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage

    assert all(unit != "abi_reduce.hip" for unit, _ in resource_usage.UNITS)
    # no unit that the kernel census compiles includes the reduction kernels
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".hpp")) and name not in ("abi_reduce.hip", "reduce.hpp"):
            assert "reduce.hpp" not in read(CSRC, name), name


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_reduce_kernels_resource_pin():
    """Exactly the shipped builds -- 2 types x 2 widths x 2 streaming flavours and the finish kernel -- each without scratch, without
    AGPRs and at 8 waves per SIMD."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage

    table = resource_usage.parse(resource_usage.compile_remarks("abi_reduce.hip"))
    want = {f"reduce_terms_kernel<{t}, {w}, {nt}>" for t, full in (("double", 2), ("float", 4)) for w in (1, full) for nt in (0, 1)}
    want.add("reduce_finish_kernel")
    got = {}
    for name, d in table.items():
        m = re.match(r"(?:void )?fus::(reduce_\w+(?:<[^>]*>)?)\(", name)
        assert m, f"a kernel that is not a reduction kernel in abi_reduce.hip: {name}"
        got[m[1]] = d
    assert set(got) == want
    for name, d in got.items():
        assert d["scratch"] == 0 and d["occupancy"] == 8 and d["agpr"] == 0, (name, d)
        assert d["lds"] == rm.WAVES * rm.SLOTS * 8, (name, d)


def test_model_constants_match_the_headers():
    shape, red = read(CSRC, "stream_shape.hpp"), read(CSRC, "reduce.hpp")
    assert re.search(r"kStreamGridCap = (\d+)", shape).group(1) == str(rm.GRID_CAP)
    m = re.search(r"kLaunchDofs = (\d+)ll << (\d+)", shape)
    assert int(m[1]) << int(m[2]) == rm.LAUNCH_DOFS
    m = re.search(r"kStreamBytes = (\d+)ll << (\d+)", shape)
    assert int(m[1]) << int(m[2]) == rm.STREAM_BYTES
    assert re.search(r"kReduceSlots = (\d+)", red).group(1) == str(rm.SLOTS)
    assert set(re.findall(r"__launch_bounds__\((\d+)\)", red)) == {str(rm.BLOCK)}
    assert re.search(r"for \(int off = (\d+); off > 0; off >>= 1\)", red).group(1) == str(rm.WAVE // 2)
    assert f"part[{rm.WAVES}][kReduceSlots]" in red and f"for (int w = 1; w < {rm.WAVES}; ++w)" in red
    assert f"i += {rm.BLOCK})" in red  # the finish kernel's chain: rows t, t + 256, ...
    assert "stream_blocks(len, decltype(w)::value, kStreamGridCap)" in red and "for_each_piece(n, kLaunchDofs" in red
    assert "atomic" not in re.sub(r"//[^\n]*", "", red)  # a fixed order: no atomics in the code


def test_model_shapes():
    assert rm.rows(0, 8, True) == 0 and rm.depth(0, 8, True) == 2 + 0 + 9 + 0 + 9 + 1
    assert rm.chain(1, 2) == 1 and rm.chain(2, 2) == 2 and rm.chain(3, 2) == 3 and rm.chain(257, 1) == 1
    big = rm.GRID_CAP * rm.BLOCK * 2 + 997  # the grid-stride loop's second, partial trip
    assert rm.blocks(big, 2) == rm.GRID_CAP and rm.chain(big, 2) == 2 * 2 + 1 and rm.chain(big, 1) == 3
    assert rm.rows(rm.LAUNCH_DOFS + 1000, 4, True) == rm.GRID_CAP + 1
    assert rm.depth(rm.LAUNCH_DOFS + 1000, 4, True) == 2 + (rm.LAUNCH_DOFS // (rm.GRID_CAP * rm.BLOCK)) + 9 + 9 + 9 + 1
