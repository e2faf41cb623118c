"""The build matrix of the streaming vector kernels (tests/stream_builds.py) on the CPU: that it names every instantiation of the ten
kernels that the library compiles, each once, and none that it does not (from the kernel names of a device-only compile: no GPU); that
its restatement of csrc/stream_shape.hpp gives the values tests/host/stream_shape_check.cpp pins; that every case's steering yields the
case's own (W, NT) through those rules; and that every case's sweep size runs the grid-stride loop a second time."""

import collections
import os
import re
import shutil
import sys

import pytest

import stream_builds as sb
from conftest import ROOT

_NAME = re.compile(r"fus::(" + "|".join(sb.KERNELS) + r")<(double|float)(?:, (.*))?>\(")


def _arg(a):
    if a in ("true", "false"):
        return a == "true"
    m = re.fullmatch(r"fus::(Op\w+)<(?:double|float)>", a)
    return m.group(1) if m else int(a)


def _compiled_keys():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    keys = []
    for name in ru.parse(ru.cached_remarks()):
        m = _NAME.search(name)
        if m:
            keys.append((m.group(1), m.group(2), tuple(_arg(a) for a in m.group(3).split(", ")) if m.group(3) else ()))
    return keys


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_the_build_matrix_is_what_the_library_compiles():
    """Every compiled instantiation of the ten kernels maps onto (kernel, type, template arguments); the matrix's cases map onto the
    same keys through ``template_key``.  The two sets are equal and neither holds a key twice: an instantiation added to the library
    without a case fails here, and so does a case that no instantiation stands behind."""
    compiled = _compiled_keys()
    tested = [sb.template_key(b) for b in sb.MATRIX]
    assert len(compiled) == len(set(compiled)) and len(tested) == len(set(tested)), "a key occurs twice"
    missing, unknown = sorted(set(compiled) - set(tested), key=repr), sorted(set(tested) - set(compiled), key=repr)
    assert not missing, f"{len(missing)} compiled instantiations have no case in the build matrix, e.g. {missing[:4]}"
    assert not unknown, f"{len(unknown)} cases of the build matrix name no compiled instantiation, e.g. {unknown[:4]}"
    assert len(compiled) == 338


def test_the_counts_per_kernel():
    assert len(sb.MATRIX) == len(set(sb.MATRIX)) == 338 and len({sb.case_id(b) for b in sb.MATRIX}) == 338
    count = collections.Counter(b.kernel for b in sb.MATRIX)
    assert dict(count) == sb.COUNTS == {"relax_stage_kernel": 96, "ew_kernel": 72, "field_accumulate_kernel": 60, "mass_gather_kernel": 48,
                                        "bioheat_stage_kernel": 24, "muladd_kernel": 12, "rk4_stage_kernel": 12, "rk4_stage_nl2_kernel": 6,
                                        "sponge_terms_kernel": 6, "rk4_stage_nl_kernel": 2}
    for k in sb.KERNELS:  # as many in either type
        assert sum(1 for b in sb.MATRIX if b.kernel == k and b.dtype == "f64") * 2 == count[k]
    # the widths: 2 doubles / 4 floats per 16-byte access, LAST of an fp32 bioheat field 2
    assert {(b.dtype, dict(b.flags)["LAST"], b.W) for b in sb.MATRIX if b.kernel == "bioheat_stage_kernel"} == {
        ("f64", False, 1), ("f64", False, 2), ("f64", True, 1), ("f64", True, 2), ("f32", False, 1), ("f32", False, 4), ("f32", True, 1), ("f32", True, 2)}
    assert {(b.dtype, b.W) for b in sb.MATRIX if b.kernel == "relax_stage_kernel"} == {("f64", 1), ("f64", 2), ("f32", 1), ("f32", 4)}


def test_the_restated_host_rules_give_the_pinned_values():
    """The literals of tests/host/stream_shape_check.cpp."""
    assert sb.STREAM_BYTES == 25165824 and sb.LAUNCH_DOFS == 134217728 and (sb.STREAM_GRID_CAP, sb.STAGE_GRID_CAP) == (2048, 4096)
    at_limit, above = (0, 0, 1, 0, 2), (0, 1, 1, 2, 2)
    for m in range(5):
        assert sb.vector_stream(25165824, m) == at_limit[m] and sb.vector_stream(25165825, m) == above[m]
        assert sb.vector_stream(0, m) == (1 if m == 2 else 2 if m == 4 else 0)
    assert sb.vector_stream(25165825) == 1 and sb.vector_stream(25165824) == 0  # the default: auto, loads and stores
    base = 4096
    assert sb.aligned16([]) and sb.aligned16([None, None, None]) and sb.aligned16([base, base + 16, base + 48])
    assert not sb.aligned16([base, base + 8, base + 32]) and not sb.aligned16([base + 4])
    assert sb.aligned16([base, None, base + 32]) and not sb.aligned16([None, base + 8])
    blocks = sb.stream_blocks
    assert blocks(1000, 2, 2048) == 2 and blocks(1000, 1, 2048) == 4 and blocks(513, 4, 2048) == 1 and blocks(513, 2, 2048) == 2
    assert blocks(1, 1, 2048) == blocks(1, 2, 2048) == blocks(1, 4, 4096) == 1 and blocks(512, 2, 2048) == 1 and blocks(514, 2, 2048) == 2
    assert blocks(10218313, 2, 4096) == 4096 and blocks(10218313, 2, 2048) == 2048
    assert blocks(1048576, 2, 2048) == 2048 and blocks(1048576, 2, 4096) == 2048 and blocks(1048064, 2, 2048) == 2047 and blocks(1048066, 2, 2048) == 2048
    assert blocks(1 << 27, 1, 4096) == 4096 and blocks((1 << 40) + 3, 1, 4096) == 4096


@pytest.mark.parametrize("b", sb.MATRIX, ids=[sb.case_id(b) for b in sb.MATRIX])
def test_steering_yields_the_build(b):
    """``steer(b)`` through the restated rules gives (W, NT) of ``b``, at the small size and at the sweep size (both far below the
    24 MiB of the auto modes: the forced modes decide); the flags a launcher switches on are the case's own."""
    s = sb.steer(b)
    assert s["offset"] in (0, 1) and s["mode"] in (0, 2, 4)
    for n in (1027, sb.sweep_size(b)):
        assert sb.chosen(b, s, n) == (b.W, b.NT), (s, n)
    for k, v in b.flags:
        assert s["mass_variant" if k == "R" else k] == v
    if b.kernel == "mass_gather_kernel":
        assert s["mode"] == (2 if b.NT else 0) and s["mass_variant"] in (1, 2, 4)
    # and the opposite alignment gives the other width, where the kernel has two
    if sb.full_width(b.kernel, b.dtype, b.flags) > 1:
        other = dict(s, offset=1 - s["offset"], odd_stride=not s.get("odd_stride", False))
        assert sb.chosen(b, other)[0] != b.W


@pytest.mark.parametrize("b", [b for b in sb.MATRIX if b.kernel != "mass_gather_kernel"],
                         ids=[sb.case_id(b) for b in sb.MATRIX if b.kernel != "mass_gather_kernel"])
def test_the_sweep_size_takes_a_second_iteration(b):
    """At the sweep size the grid is at its cap, at least one and fewer than gridDim x 256 threads take a second iteration of the
    grid-stride loop, and a wide build is left a scalar tail.  The largest case is the fp32 aligned rk4_stage_kernel's."""
    n, cap = sb.sweep_size(b), sb.grid_cap(b.kernel)
    assert sb.stream_blocks(n, b.W, cap) == cap and cap == (4096 if b.kernel.startswith("rk4_stage") else 2048)
    assert 0 < sb.second_sweep_threads(b) < cap * 256 and sb.second_sweep_threads(b) in (777, 778)
    if b.W > 1:
        assert n % b.W != 0
    for nlocal in (n, n - 5):  # the kernels with an owned range run it 5 short of n
        assert (nlocal // b.W) > cap * 256
    assert n <= 4_197_413 and n * sb.ITEMSIZE[b.dtype] < sb.STREAM_BYTES and n < sb.LAUNCH_DOFS


def test_the_gather_sweep_sizes():
    """57 row blocks in chunks of 8 per XCD: every chunk holds a live block, 7 workgroups return, the last live one is partly filled."""
    for r in (1, 2, 4):
        nrows = sb.gather_rows(r)
        nkb = -(-nrows // (256 * r))
        chunk = -(-nkb // 8)
        assert nrows > 8 * 256 * r and nrows % (256 * r) != 0
        live = [[x * chunk + j < nkb for j in range(chunk)] for x in range(8)]
        assert all(any(row) for row in live) and sum(not v for row in live for v in row) == 7
