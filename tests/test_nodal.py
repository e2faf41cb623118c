"""Nodal material fields, the parts that need no GPU: ``nodal_medium`` (``scale_G``, ``sample_volume``, the ``NodalMedium`` checks), the
operator's keyword check, the binding's open header tier with the two new entry points, and the register allocation of the new kernels
(hipcc cross-compiles gfx950 without a GPU).  The kernel and the solver run in tests/test_nodal_gpu.py."""

import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import nodal_cpu
from conftest import build_problem, pkg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- nodal_medium ------------------------------------------------------------------------------------------------------------------
def test_scale_G_of_a_constant_is_the_constant_times_G():
    import torch

    nm = pkg("nodal_medium")
    pb = build_problem(2, (2, 2, 1), perturb=0.1)
    mesh, G = pb["mesh"], torch.from_numpy(pb["G"])
    got = nm.scale_G(G, np.full(mesh.ndofs, 2.5), mesh.dofmap)
    assert got.dtype == G.dtype and got.shape == G.shape and got.is_contiguous()
    assert np.array_equal(got.numpy(), 2.5 * pb["G"])
    # ... and of a field: the model's array (tests/nodal_cpu.py), bit for bit (one product per entry on either side)
    kappa = nodal_cpu.smooth_field(mesh.dof_coordinates(), 1.0, 3.0, 1.0)
    assert np.array_equal(nm.scale_G(G, kappa, torch.from_numpy(mesh.dofmap)).numpy(), nodal_cpu.scaled_G(pb["G"], kappa, mesh.dofmap))
    with pytest.raises(ValueError):
        nm.scale_G(G, kappa[:-1], mesh.dofmap)  # a dof beyond kappa
    with pytest.raises(ValueError):
        nm.scale_G(G[:, :, :5], kappa, mesh.dofmap)
    with pytest.raises(TypeError):
        nm.scale_G(pb["G"], kappa, mesh.dofmap)


def test_sample_volume_is_trilinear_and_clamps():
    nm = pkg("nodal_medium")
    origin, spacing = np.array([0.1, -0.2, 0.05]), np.array([0.01, 0.02, 0.005])
    shape = (5, 4, 7)
    ijk = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij"), axis=-1)
    xyz = origin + ijk * spacing
    f = lambda p: 1.0 + 2.0 * p[..., 0] - 3.0 * p[..., 1] + 5.0 * p[..., 2] + 40.0 * p[..., 0] * p[..., 1] * p[..., 2] + 7.0 * p[..., 1] * p[..., 2]  # noqa: E731
    vol = f(xyz)  # trilinear: reproduced exactly (to rounding) anywhere inside the volume
    rng = np.random.default_rng(0)
    hi = origin + (np.array(shape) - 1) * spacing
    pts = origin + rng.random((200, 3)) * (hi - origin)
    pts = np.concatenate([pts, xyz.reshape(-1, 3)[::7], [origin, hi]])  # the voxel points and the two corners among them
    got = nm.sample_volume(vol, origin, spacing, pts)
    assert np.max(np.abs(got - f(pts))) < 1e-13 * np.max(np.abs(vol))
    # outside: the value at the nearest point of the faces
    out = np.array([[origin[0] - 1.0, pts[3, 1], pts[3, 2]], [hi[0] + 0.3, hi[1] + 0.3, pts[5, 2]], origin - 1.0, hi + 1.0])
    clamped = np.clip(out, origin, hi)
    assert np.max(np.abs(nm.sample_volume(vol, origin, spacing, out) - f(clamped))) < 1e-13 * np.max(np.abs(vol))
    # a scalar spacing, a one-voxel axis, and the argument checks
    assert nm.sample_volume(np.full((1, 3, 3), 4.0), 0.0, 1.0, [[0.5, 1.2, 7.0]])[0] == 4.0
    for bad in (lambda: nm.sample_volume(vol[0], origin, spacing, pts), lambda: nm.sample_volume(vol, origin, spacing, pts[:, :2]),
                lambda: nm.sample_volume(vol, origin, [0.01, 0.0, 0.01], pts)):
        with pytest.raises(ValueError):
            bad()


class _NoCoordinates:
    """A mesh as handed over in arrays: no ``dof_coordinates``."""

    def __init__(self, mesh):
        self.ndofs, self.dofmap = mesh.ndofs, mesh.dofmap


def test_nodal_medium_checks():
    nm = pkg("nodal_medium")
    mesh = build_problem(2, (2, 1, 1))["mesh"]
    nd = mesh.ndofs
    c, rho = nm.NodalMedium(1500.0, lambda xyz: 1000.0 + 100.0 * xyz[:, 0]).evaluate(mesh)
    assert c.shape == (nd,) and np.all(c == 1500.0) and c.dtype == np.float64
    assert np.array_equal(rho, 1000.0 + 100.0 * mesh.dof_coordinates()[:, 0])
    arr = np.linspace(1400.0, 1600.0, nd)
    assert np.array_equal(nm.NodalMedium(arr, 1000.0).evaluate(mesh)[0], arr)
    bare = _NoCoordinates(mesh)
    assert np.array_equal(nm.NodalMedium(arr, 1000.0).evaluate(bare)[0], arr)  # arrays and scalars need no coordinates
    with pytest.raises(ValueError, match="dof_coordinates"):
        nm.NodalMedium(lambda xyz: arr, 1000.0).evaluate(bare)
    with pytest.raises(ValueError, match="one value per local dof"):
        nm.NodalMedium(arr[:-1], 1000.0).evaluate(mesh)
    with pytest.raises(ValueError, match="one value per local dof"):
        nm.NodalMedium(1500.0, lambda xyz: np.ones(3)).evaluate(mesh)
    for bad in (np.nan, np.inf, 0.0, -1.0):
        a = arr.copy()
        a[3] = bad
        with pytest.raises(ValueError, match="non-finite|positive"):
            nm.NodalMedium(a, 1000.0).evaluate(mesh)
        with pytest.raises(ValueError, match="non-finite|positive"):
            nm.NodalMedium(1500.0, a).evaluate(mesh)
    # the per-cell and per-facet means the solver derives
    assert np.allclose(nm.cell_means(arr, mesh.dofmap), arr[mesh.dofmap].mean(axis=1))
    fd = mesh.facet_dofmap(mesh.boundary_facets([2]))
    assert np.array_equal(nm.facet_means(np.full(nd, 3.0), fd), np.full(fd.shape[0], 3.0)) and nm.facet_means(arr, fd[:0]).shape == (0,)


def test_nodal_keyword_needs_in_kernel_geometry():
    """Without ``geometry`` the operator is a general-G one: ``nodal=`` raises before anything touches a device and points to scale_G."""
    ops = pkg("operators")
    pb = build_problem(2, (2, 1, 1))
    with pytest.raises(ValueError, match="nodal_medium.scale_G"):
        ops.stiffness_operator(2, pb["D"].flatten(), np.float64, nodal=np.ones(pb["mesh"].ndofs))
    with pytest.raises(ValueError, match="nodal_medium.scale_G"):
        ops.stiffness_operator(2, np.float64, nodal=np.ones(pb["mesh"].ndofs))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
NAMES = ("fus_stiffness_apply_planned_geom_nodal_f64", "fus_stiffness_apply_planned_geom_nodal_f32")


def test_binding_declares_the_entry_points():
    """The two entry points come from include/fus_gpu_nodal.h through the header parser into the binding's open tier (``_lib.LATER``:
    every later header goes there); they are the geometry apply's arguments with ``nodal`` after ``cell_constants``; the library
    exports them, include/fus_gpu.hpp includes the header, the ABI version stays 3, and the three older sets are what they were."""
    lib_mod = pkg("_lib")
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    for name in NAMES:
        assert lib_mod.LATER[name] == (i, [vp] * 10 + [i, i64, vp])
        geom = lib_mod.DECLARATIONS[name.replace("_nodal", "")][1]
        assert lib_mod.LATER[name][1] == geom[:2] + [vp] + geom[2:]
    assert not set(lib_mod.LATER) & (set(lib_mod.DECLARATIONS) | set(lib_mod.EXTENSIONS) | set(lib_mod.ADDITIONS))
    assert any(p.endswith("fus_gpu_nodal.h") for p in lib_mod.LATER_HEADER_PATHS)
    hdr = open(os.path.join(ROOT, "include", "fus_gpu_nodal.h")).read()
    assert '#include "fus_gpu.h"' in hdr and all(name in hdr for name in NAMES)
    assert '#include "fus_gpu_nodal.h"' in open(os.path.join(ROOT, "include", "fus_gpu.hpp")).read()
    # the pinned sets did not grow
    assert len(lib_mod.DECLARATIONS) == 125 and len(lib_mod.SIGNATURES) == 123
    assert len(lib_mod.EXTENSIONS) == 4 and set(lib_mod.ADDITIONS) == {"fus_relax_stage_f64", "fus_relax_stage_f32"}
    lib = lib_mod.load()
    assert lib_mod.ABI_VERSION == 3 and lib.fus_abi_version() == 3
    for name in NAMES:
        fn = getattr(lib, name)  # exported
        assert list(fn.argtypes) == lib_mod.LATER[name][1] and fn.restype is i
    # the checks that come before any device work, in the order of the geometry apply's
    z, one = C.c_void_p(0), C.c_void_p(256)
    call = lambda P, ncell, nodal=one, ws=one: lib.fus_stiffness_apply_planned_geom_nodal_f64(one, one, nodal, one, one, one, one, one, ws, one, P, ncell, z)  # noqa: E731
    assert call(4, -1) == -1 and call(0, 5) == lib_mod._DEFINES["FUS_ERR_UNSUPPORTED_DEGREE"] and call(11, 5) == lib_mod._DEFINES["FUS_ERR_UNSUPPORTED_DEGREE"]
    assert call(4, 0, z, z) == 0  # the empty mesh: before any pointer is looked at
    assert call(4, 5, z) == -1 and call(4, 5, one, z) == -1  # a null coefficient, a null workspace
    assert call(4, 5) == lib_mod._DEFINES["FUS_ERR_PLAN_MISMATCH"]  # no plan is registered at that address


def test_a_duplicate_declaration_in_a_later_header_is_refused(tmp_path):
    """The open tier has the duplicate check of the older ones: a later header may not declare what an earlier tier, or a header
    before it in the tier, declares."""
    lib_mod = pkg("_lib")
    earlier = set(lib_mod.DECLARATIONS) | set(lib_mod.EXTENSIONS) | set(lib_mod.ADDITIONS)
    assert lib_mod.declared_later(lib_mod.LATER_HEADER_PATHS, earlier) == lib_mod.LATER
    fresh = tmp_path / "fus_gpu_fresh.h"
    fresh.write_text('#include "fus_gpu.h"\nint fus_something_new_f64(const double* x, int64_t n, void* stream);\n')
    tier = lib_mod.declared_later(lib_mod.LATER_HEADER_PATHS + (str(fresh),), earlier)
    assert tier["fus_something_new_f64"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]) and set(lib_mod.LATER) < set(tier)
    for text in ("int fus_abi_version(void);\n", "int fus_relax_stage_f64(void* x);\n", f"int {NAMES[0]}(void* x);\n"):
        dup = tmp_path / "fus_gpu_dup.h"
        dup.write_text('#include "fus_gpu.h"\n' + text)
        with pytest.raises(lib_mod.FusGpuError, match="two headers"):
            lib_mod.declared_later(lib_mod.LATER_HEADER_PATHS + (str(dup),), earlier)


def test_the_cpp_functor_compiles_in_both_types(tmp_path):
    """include/fus_gpu.hpp's NodalStiffnessSpectral3D through the compiler (host pass only, no GPU, no library): its typed forward
    against the prototypes of include/fus_gpu_nodal.h, for double and float and P = 1, 4, 10."""
    import subprocess

    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "tests", "host", "fus_gpu_nodal_check.cpp")
    b = subprocess.run([hipcc, "--cuda-host-only", "-c", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(tmp_path / "check.o"), src],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]


def test_the_timing_tool_parses_its_arguments_before_any_work():
    """tools/time_nodal.py --help in a fresh child process on a machine without a GPU (as tests/test_measure.py asks of every tool
    built on tools/measure.py)."""
    import subprocess

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_nodal.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--configs" in r.stdout and "pre-scaled G" in r.stdout


# ---- the kernels' resources --------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_nodal_kernel_resources():
    """Every instantiation of stiffness_plan_geom_nodal_kernel (2 types x 10 degrees x 4 (ORDERED, RUNS) shapes = 80): no scratch, no
    AGPRs, and at least the waves per SIMD of westervelt_cell_geom_kernel<..., MASS = false, ...> -- the existing two-gather cell pass
    with in-kernel geometry -- at the same degree, type and shape; fp64 P = 4 keeps the four waves of the per-cell kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    table = ru.parse(ru.cached_remarks())
    nodal = {k: v for k, v in table.items() if "stiffness_plan_geom_nodal_kernel<" in k}
    assert len(nodal) == 80, sorted(nodal)
    seen = set()
    for name, d in nodal.items():
        m = re.search(r"nodal_kernel<(double|float), (\d+), (\d+), (?:true|false), (?:true|false), \d+, (?:true|false), (true|false), (true|false)>", name)
        assert m, name
        t, P, cpb, o, r = m.groups()
        seen.add((t, int(P), o, r))
        assert d["scratch"] == 0 and d["agpr"] == 0, (name, d)
        twin = [v for k, v in table.items() if f"westervelt_cell_geom_kernel<{t}, {P}, {cpb}, 1, false, {o}, {r}>" in k]
        assert len(twin) == 1, (name, len(twin))
        assert d["occupancy"] >= twin[0]["occupancy"], (name, d, twin[0])
        assert d["lds"] <= twin[0]["lds"] or d["occupancy"] >= twin[0]["occupancy"]
    assert len(seen) == 80 and {p for _, p, _, _ in seen} == set(range(1, 11))
    for o in ("false", "true"):
        for r in ("false", "true"):
            hits = [v for k, v in table.items() if re.search(rf"stiffness_plan_geom_nodal_kernel<double, 4, 10, true, true, \d+, true, {o}, {r}>", k)]
            percell = [v for k, v in table.items() if f"stiffness_plan_geom_kernel<double, 4, 10, true, true, 1, true, {o}, {r}>" in k]
            assert len(hits) == 1 and len(percell) == 1
            assert hits[0]["vgpr"] <= 128 and hits[0]["occupancy"] >= percell[0]["occupancy"] >= 4 and hits[0]["lds"] == percell[0]["lds"]
