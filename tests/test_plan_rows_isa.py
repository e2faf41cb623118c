"""The compiled shape of ``stiffness_plan_rows_kernel`` (csrc/stiffness_plan.hpp: the general-G kernel that reads one slot per local row
and the compact run tables), no GPU needed:
  * load and wait ORDER of its preamble, the rules of csrc/plan.hpp as tests/test_kernel_isa.py states them for ``stiffness_plan_kernel``
    -- the whole G slab, the run words, the dphi entry and the n row-base loads go out before the first vector wait, that wait leaves
    the slab in flight, and nothing waits for "everything" before the x gather;
  * every degree the dispatch ships it for (csrc/dispatch_stiffness_plan.hip: plan_rows_ships) has no scratch, and the registers,
    occupancy and LDS its ``stiffness_plan_kernel`` twin has -- the condition under which a degree takes it."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the pins of load order were taken with this compiler; on another release a failing order is an expected failure (test_kernel_isa.py)
PINNED_HIP_VERSION = "7.2.26015"


def _hip_version():
    try:
        out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    except OSError:
        return None
    m = re.search(r"HIP version:\s*([0-9.]+)", out)
    return m.group(1) if m else None


_have_hipcc = shutil.which("hipcc") is not None or os.path.exists(HIPCC)
_pinned = _have_hipcc and _hip_version() == PINNED_HIP_VERSION
pytestmark = pytest.mark.skipif(not _have_hipcc, reason="hipcc not available")

SOURCE = r"""
#include "stiffness_plan.hpp"
namespace fus {
template __global__ void stiffness_plan_rows_kernel<double, 4, 10, true, true, 1, 5, false, true>(const double*, const double*, double*, const double*, const int32_t*, const int32_t*, const uint16_t*, const double*, int64_t, int, const int32_t*, const int32_t*, int, LaunchSignal);
}
"""


@pytest.fixture(scope="module")
def rows_kernel():
    """instruction lines of the fp64 P = 4 rows kernel (un-ordered plan, run tables: what the headline launches)"""
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "rows.hip"), os.path.join(d, "rows.s")
        with open(src, "w") as f:
            f.write(SOURCE)
        cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=fast", "-fno-slp-vectorize",
               "--cuda-device-only", "-S", "-I" + CSRC, "-o", out, src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        text = open(out).read().split("\n")
    lines, inside = [], False
    for ln in text:
        if re.match(r"^_ZN3fus26stiffness_plan_rows_kernelIdLi4E\w*:", ln):
            inside = True
            continue
        if inside:
            s = ln.strip()
            if s and not s.startswith((";", ".")):
                lines.append(s)
            if s.startswith("s_endpgm"):
                break
    assert lines and lines[-1].startswith("s_endpgm")
    return lines


def _vm_wait(s):
    m = re.match(r"s_waitcnt .*vmcnt\((\d+)\)", s)
    return int(m.group(1)) if m else None


def _is_load(s):
    return s.startswith(("global_load", "flat_load"))


@pytest.mark.xfail(condition=not _pinned, strict=False,
                   reason=f"ISA pins were taken with HIP {PINNED_HIP_VERSION}; this is {_hip_version()}: scheduling may differ")
def test_rows_kernel_issues_everything_before_its_first_wait(rows_kernel):
    k = rows_kernel
    first_wait = next(i for i, s in enumerate(k) if _vm_wait(s) is not None)
    before = [s for s in k[:first_wait] if _is_load(s)]
    slab = [s for s in before if s.startswith("global_load_dwordx4")]
    assert len(slab) == 15, f"the whole G slab (5 planes x 3 x 16 bytes) must be in flight before the first wait, found {len(slab)}"
    bases = [s for s in before if s.startswith("global_load_ushort")]
    assert len(bases) == 5, f"the five row bases, as 16-bit loads into 32-bit words: {before}"
    assert len(before) >= 15 + 1 + 3 + 5, before  # + the dphi entry, the three run words, the five row bases
    assert _vm_wait(k[first_wait]) >= 15, f"the first wait must leave the G slab in flight: {k[first_wait]}"
    # after the barrier of the run expansion: the x gather goes out before anything waits for every outstanding load
    barrier = next(i for i, s in enumerate(k) if s.startswith("s_barrier"))
    after = k[barrier:]
    gather = next(i for i, s in enumerate(after) if s.startswith("global_load_dwordx2"))
    assert all(_vm_wait(s) != 0 for s in after[:gather]), "a full wait before the x gather: the G slab would be waited for first"


# (rows kernel, its stiffness_plan_kernel twin): the auto build of each degree the dispatch ships the rows kernel for, un-ordered and
# ordered plans; the last template argument (RUNS) is true, the only form launched
_BUILDS = {2: "2, 28, false, true, 1, 3", 3: "3, 16, false, true, 1, 4", 4: "4, 10, true, true, 1, 5", 5: "5, 7, true, true, 1, 6",
           6: "6, 5, true, true, 1, 4", 7: "7, 4, true, true, 1, 3", 8: "8, 3, true, false, 1, 2"}


@pytest.fixture(scope="module")
def table():
    import resource_usage as ru

    return ru.parse(ru.cached_remarks())


def _find(table, pattern):
    hits = [v for k, v in table.items() if re.search(pattern, k)]
    assert len(hits) == 1, f"{pattern!r} matches {len(hits)} kernels"
    return hits[0]


@pytest.mark.parametrize("P", sorted(_BUILDS))
def test_rows_kernel_keeps_the_resources_of_its_twin(table, P):
    for ordered in ("false", "true"):
        rows = _find(table, rf"stiffness_plan_rows_kernel<double, {_BUILDS[P]}, {ordered}, true>")
        twin = _find(table, rf"stiffness_plan_kernel<double, {_BUILDS[P]}, {ordered}, true>")
        assert rows["scratch"] == 0 and rows["agpr"] == 0, rows
        assert rows["occupancy"] >= twin["occupancy"] and rows["lds"] <= twin["lds"], (P, rows, twin)
    if P == 4:  # the headline: 4 waves per SIMD by registers, 4 workgroups per CU by LDS
        assert rows["vgpr"] <= 128 and rows["occupancy"] >= 4 and 4 * rows["lds"] <= 160 * 1024, rows


def test_only_shipped_degrees_are_instantiated(table):
    """the library holds a rows kernel for exactly the degrees listed above, fp64 only"""
    got = sorted({int(re.search(r"rows_kernel<double, (\d+),", k).group(1)) for k in table if "stiffness_plan_rows_kernel<double" in k})
    assert got == sorted(_BUILDS), got
    assert not [k for k in table if "stiffness_plan_rows_kernel<float" in k]
