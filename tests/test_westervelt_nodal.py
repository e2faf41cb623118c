"""The Westervelt solver with a nodal medium, the parts that need no GPU: the CPU model (tests/westervelt_nodal_cpu.py) against the
oracle the reference pins, ``NodalMedium``'s two new fields, the binding of the two new entry points, the host compile check of the
functor, the operator's keyword check, the register allocation of the new kernel (hipcc cross-compiles gfx950 without a GPU) and the
timing tool's ``--help``.  The kernel and the solver run in tests/test_westervelt_nodal_gpu.py."""

import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import westervelt_nodal_cpu
from conftest import build_problem, pkg, rel_l2
from oracle import rk4_oracle

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the CPU model -----------------------------------------------------------------------------------------------------------------
def test_model_with_constant_nodal_values_is_the_oracle():
    """Constant nodal values: the model equals ``rk4_oracle.solve_westervelt`` with the same scalars to 1e-13 over 10 steps (perturbed
    cells, P = 3) -- stiffness on the scaled G, the three diagonals from M(1) 1, the facet means and the reference scalars all reduce."""
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    P, L = 3, 0.006
    mesh = boxmesh.BoxMesh(P, (3, 2, 2), length=L, perturb=0.1, seed=5)
    dt = ls.snap_time_step(ls.time_step_parameters(mesh, P, 1540.0, 1.1e6, L), P, 1540.0, 1.1e6, L)[0]
    kw = dict(c0=1540.0, rho0=1050.0, beta=4.2, att_dB=0.7)
    u_ref, v_ref = rk4_oracle.solve_westervelt(mesh, 10, dt, **kw)
    nd = mesh.ndofs
    for fields in ((1540.0, 1050.0, 4.2, 0.7), tuple(np.full(nd, a) for a in (1540.0, 1050.0, 4.2, 0.7))):
        u, v = westervelt_nodal_cpu.solve(mesh, 10, dt, *fields)
        du, dv = rel_l2(u, u_ref), rel_l2(v, v_ref)
        print(f"constant nodal values against the oracle: u {du:.3e} v {dv:.3e}")
        assert np.max(np.abs(u_ref)) > 0 and du < 1e-13 and dv < 1e-13


def test_model_stiffness_pair_is_two_scaled_applies():
    """``stiffness_pair`` against the definition, cell by cell: sum_q B^T G (c3 k3 grad u + c4 k4 grad v) = K(G c3 k3) u + K(G c4 k4) v,
    and swapping the two coefficient fields changes the result."""
    from oracle import oracle_np

    pb = build_problem(2, (2, 2, 1), perturb=0.15, seed=3)
    mesh = pb["mesh"]
    rng = np.random.default_rng(0)
    k3, k4 = 1.0 + 2.0 * rng.random(mesh.ndofs), 1.0 + 2.0 * rng.random(mesh.ndofs)
    u, v = pb["x"], rng.standard_normal(mesh.ndofs)
    c3, c4 = pb["cc"], 0.5 + rng.random(mesh.ncells)
    b = np.zeros(mesh.ndofs)
    westervelt_nodal_cpu.stiffness_pair(2, pb["D"], u, v, c3, c4, b, pb["G"], mesh.dofmap, k3, k4)
    ref = np.zeros(mesh.ndofs)
    G34 = pb["G"] * (c3[:, None] * k3[mesh.dofmap])[:, :, None]
    oracle_np.stiffness_apply(2, pb["D"].flatten(), u, np.ones(mesh.ncells), ref, G34, mesh.dofmap)
    G34 = pb["G"] * (c4[:, None] * k4[mesh.dofmap])[:, :, None]
    oracle_np.stiffness_apply(2, pb["D"].flatten(), v, np.ones(mesh.ncells), ref, G34, mesh.dofmap)
    assert rel_l2(b, ref) < 1e-14
    swapped = np.zeros(mesh.ndofs)
    westervelt_nodal_cpu.stiffness_pair(2, pb["D"], u, v, c3, c4, swapped, pb["G"], mesh.dofmap, k4, k3)
    assert rel_l2(swapped, ref) > 1e-2


# ---- NodalMedium -------------------------------------------------------------------------------------------------------------------
def test_nodal_medium_westervelt_fields():
    nm = pkg("nodal_medium")
    mesh = build_problem(2, (2, 1, 1))["mesh"]
    nd = mesh.ndofs
    xyz = mesh.dof_coordinates()
    arr = np.linspace(0.0, 2.0, nd)  # alpha = 0 is a lossless region: allowed
    m = nm.NodalMedium(1500.0, 1000.0, nonlinear_coefficient=lambda p: 3.5 + p[:, 0], attenuation_coefficient_dB=arr)
    c, rho, beta, att = m.evaluate_westervelt(mesh)
    assert all(a.shape == (nd,) and a.dtype == np.float64 for a in (c, rho, beta, att))
    assert np.all(c == 1500.0) and np.all(rho == 1000.0) and np.array_equal(beta, 3.5 + xyz[:, 0]) and np.array_equal(att, arr)
    # a field left None takes the scalar handed over; None in both places raises
    c, rho, beta, att = nm.NodalMedium(1500.0, 1000.0, attenuation_coefficient_dB=0.5).evaluate_westervelt(mesh, 4.0, 0.2)
    assert np.all(beta == 4.0) and np.all(att == 0.5)
    with pytest.raises(ValueError, match="nonlinear_coefficient"):
        nm.NodalMedium(1500.0, 1000.0).evaluate_westervelt(mesh, None, 0.2)
    with pytest.raises(ValueError, match="attenuation_coefficient_dB"):
        nm.NodalMedium(1500.0, 1000.0, nonlinear_coefficient=3.5).evaluate_westervelt(mesh)
    # shapes, callables, negative and non-finite values
    with pytest.raises(ValueError, match="one value per local dof"):
        nm.NodalMedium(1500.0, 1000.0, nonlinear_coefficient=arr[:-1]).evaluate_westervelt(mesh, 3.5, 0.2)
    with pytest.raises(ValueError, match="one value per local dof"):
        nm.NodalMedium(1500.0, 1000.0, attenuation_coefficient_dB=lambda p: np.ones(3)).evaluate_westervelt(mesh, 3.5, 0.2)
    for bad in (np.nan, np.inf, -1e-3):
        a = 1.0 + arr
        a[3] = bad
        for kw in (dict(nonlinear_coefficient=a), dict(attenuation_coefficient_dB=a)):
            with pytest.raises(ValueError, match="non-finite|negative"):
                nm.NodalMedium(1500.0, 1000.0, **kw).evaluate_westervelt(mesh, 3.5, 0.2)
    with pytest.raises(TypeError):
        nm.NodalMedium(1500.0, 1000.0, 3.5)  # the new fields are keywords
    # the old two-argument form and evaluate() are what they were: (c, rho), positive values only, the new fields ignored
    old = nm.NodalMedium(np.linspace(1400.0, 1600.0, nd), lambda p: 1000.0 + 100.0 * p[:, 0])
    assert old.nonlinear_coefficient is None and old.attenuation_coefficient_dB is None
    out = old.evaluate(mesh)
    assert len(out) == 2 and np.array_equal(out[0], np.linspace(1400.0, 1600.0, nd)) and np.array_equal(out[1], 1000.0 + 100.0 * xyz[:, 0])
    assert len(m.evaluate(mesh)) == 2
    with pytest.raises(ValueError, match="positive"):
        nm.NodalMedium(0.0, 1000.0).evaluate(mesh)


# ---- the operator's keyword ----------------------------------------------------------------------------------------------------------
def test_nodal_keyword_needs_in_kernel_geometry():
    """``nodal=`` without ``geometry=`` raises before anything touches a device."""
    ops = pkg("operators")
    pb = build_problem(2, (2, 1, 1))
    ones = np.ones(pb["mesh"].ndofs)
    with pytest.raises(ValueError, match="needs geometry"):
        ops.westervelt_cell_operator(2, pb["D"].flatten(), np.float64, nodal=(ones, ones))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
NAMES = ("fus_westervelt_stiffness_apply_planned_geom_nodal_f64", "fus_westervelt_stiffness_apply_planned_geom_nodal_f32")


def test_binding_declares_the_entry_points():
    """The two entry points come from include/fus_gpu_westervelt_nodal.h through the header parser into ``_lib.LATER``: u, v, c3, c4,
    nodal3, nodal4, b, then the geometry apply's tail; the library exports them, include/fus_gpu.hpp includes the header, the ABI
    version stays 3 and the pinned sets are what they were.  Then the checks that come before any device work, in their order."""
    lib_mod = pkg("_lib")
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    for name in NAMES:
        assert lib_mod.LATER[name] == (i, [vp] * 13 + [i, i64, vp])
        nodal = lib_mod.LATER[name.replace("westervelt_", "")][1]  # (x, cc, nodal, y, x_g, x_dofs, pts, wts, ws, dphi, P, ncell, stream)
        assert lib_mod.LATER[name][1] == [vp] * 7 + nodal[4:]
    assert not set(lib_mod.LATER) & (set(lib_mod.DECLARATIONS) | set(lib_mod.EXTENSIONS) | set(lib_mod.ADDITIONS))
    assert any(p.endswith("fus_gpu_westervelt_nodal.h") for p in lib_mod.LATER_HEADER_PATHS)
    hdr = open(os.path.join(ROOT, "include", "fus_gpu_westervelt_nodal.h")).read()
    assert '#include "fus_gpu.h"' in hdr and all(name in hdr for name in NAMES)
    for arg in ("u", "v", "c3", "c4", "nodal3", "nodal4", "b", "x_g", "x_dofs", "pts", "wts", "workspace", "dphi", "P", "ncell", "stream"):
        assert re.search(rf"\b{arg}\b", hdr), arg
    order = re.search(r"_f64\((.*?)\);", hdr, re.S).group(1)
    names = [re.sub(r".*[ *]", "", a.strip()) for a in order.split(",")]
    assert names == ["u", "v", "c3", "c4", "nodal3", "nodal4", "b", "x_g", "x_dofs", "pts", "wts", "workspace", "dphi", "P", "ncell", "stream"]
    assert '#include "fus_gpu_westervelt_nodal.h"' in open(os.path.join(ROOT, "include", "fus_gpu.hpp")).read()
    # the pinned sets did not grow
    assert len(lib_mod.DECLARATIONS) == 125 and len(lib_mod.EXTENSIONS) == 4
    assert set(lib_mod.ADDITIONS) == {"fus_relax_stage_f64", "fus_relax_stage_f32"}
    lib = lib_mod.load()
    assert lib_mod.ABI_VERSION == 3 and lib.fus_abi_version() == 3
    for name in NAMES:
        fn = getattr(lib, name)  # exported
        assert list(fn.argtypes) == lib_mod.LATER[name][1] and fn.restype is i
    z, one = C.c_void_p(0), C.c_void_p(256)
    for fn in (getattr(lib, n) for n in NAMES):
        call = lambda P, ncell, n3=one, n4=one, ws=one, u=one: fn(u, one, one, one, n3, n4, one, one, one, one, one, ws, one, P, ncell, z)  # noqa: E731,B023
        unsupported = lib_mod._DEFINES["FUS_ERR_UNSUPPORTED_DEGREE"]
        assert call(4, -1) == -1 and call(0, 5) == unsupported and call(11, 5) == unsupported
        assert call(4, -1, z, z, z) == -1 and call(11, 5, z, z, z) == unsupported  # ... both before any pointer is looked at
        assert call(4, 0, z, z, z, z) == 0  # the empty mesh: before any pointer is looked at
        assert call(4, 5, z) == -1 and call(4, 5, one, z) == -1 and call(4, 5, u=z) == -1  # null coefficients, a null input
        assert call(4, 5, ws=z) == -1  # a null workspace
        assert call(4, 5) == lib_mod._DEFINES["FUS_ERR_PLAN_MISMATCH"]  # no plan is registered at that address


def test_the_cpp_functor_compiles_in_both_types(tmp_path):
    """include/fus_gpu.hpp's WesterveltNodalStiffnessSpectral3D through the compiler (host pass only, no GPU, no library)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "tests", "host", "fus_gpu_westervelt_nodal_check.cpp")
    b = subprocess.run([hipcc, "--cuda-host-only", "-c", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(tmp_path / "check.o"), src],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]


def test_the_timing_tool_parses_its_arguments_before_any_work():
    """tools/time_westervelt_nodal.py --help in a fresh child process on a machine without a GPU."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_westervelt_nodal.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--configs" in r.stdout and "two launches" in r.stdout


def test_the_build_lists_the_new_unit():
    mk = open(os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc", "Makefile")).read()
    assert mk.count("dispatch_westervelt_nodal") == 2 and "westervelt_geom_nodal.hpp" in mk and "fus_gpu_westervelt_nodal.h" in mk
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    assert ("dispatch_westervelt_nodal.hip", ("-DFUS_INST_T=double",)) in ru.UNITS and ("dispatch_westervelt_nodal.hip", ("-DFUS_INST_T=float",)) in ru.UNITS


# ---- the kernel's resources --------------------------------------------------------------------------------------------------------
LDS_LIMIT = 160 * 1024  # bytes of LDS a workgroup can be given on gfx950


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_westervelt_nodal_kernel_resources():
    """Every instantiation of westervelt_cell_geom_nodal_kernel (2 types x 10 degrees x 4 (ORDERED, RUNS) shapes = 80): present, no
    scratch, no AGPRs, static LDS within the limit -- and, the form being the three-cube one, no more LDS than its per-cell twin
    westervelt_cell_geom_kernel<..., MASS = false, ...> at the same degree, type and shape.  The existing kernels keep their names."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    table = ru.parse(ru.cached_remarks())
    new = {k: v for k, v in table.items() if "westervelt_cell_geom_nodal_kernel<" in k}
    assert len(new) == 80, sorted(new)
    seen = set()
    for name, d in new.items():
        assert "stiffness_plan_geom_nodal_kernel<" not in name and "westervelt_cell_geom_kernel<" not in name
        m = re.search(r"nodal_kernel<(double|float), (\d+), (\d+), (\d+), (true|false), (true|false)>", name)
        assert m, name
        t, P, cpb, _, o, r = m.groups()
        seen.add((t, int(P), o, r))
        assert d["scratch"] == 0 and d["agpr"] == 0, (name, d)
        assert 0 < d["lds"] <= LDS_LIMIT and d["vgpr"] <= 256 and d["occupancy"] >= 2, (name, d)
        twin = [v for k, v in table.items() if f"westervelt_cell_geom_kernel<{t}, {P}, {cpb}, 1, false, {o}, {r}>" in k]
        assert len(twin) == 1, (name, len(twin))
        assert d["lds"] <= twin[0]["lds"], (name, d, twin[0])
    assert len(seen) == 80 and {p for _, p, _, _ in seen} == set(range(1, 11))
    # the counts the existing resource tests take by substring are what they were
    assert len([k for k in table if "stiffness_plan_geom_nodal_kernel<" in k]) == 80
    assert len([k for k in table if "westervelt_cell_geom_kernel<" in k]) == 160
