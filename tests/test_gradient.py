"""The gradient cell operator and the maps built on it (intensity.py), the parts that need no GPU: the numpy restatement the GPU
tests compare with (tests/gradient_cpu.py) anchored to reference-held data and to closed forms, the new symbols in the header and
the binding, argument validation before any device work, and the register / LDS / occupancy table of the new kernel."""

import ctypes as C
import os
import re
import shutil
import sys
import types

import numpy as np
import pytest

import gradient_cpu as gc
from conftest import GOLDEN, ROOT, TOL, golden_files, pkg, rel_l2, rel_max

sys.path.insert(0, os.path.join(ROOT, "tools"))
intensity = pkg("intensity")  # (every test of this module is about the feature: none runs without it)

ANCHORS = [f for f in golden_files("ops_") if f.endswith("_pert_float64.npz")] + [os.path.join(GOLDEN, "ops_P2_3x2x2_affine_float64.npz")]


# ---- 1. the restatement against what the reference computed ----------------------------------------------------------------
@pytest.mark.parametrize("path", ANCHORS, ids=[os.path.basename(f)[4:-4] for f in ANCHORS])
def test_restatement_reproduces_the_reference_factors_and_stiffness(path):
    """w |det| == ref_detJ, w |det| inv^T inv == ref_G, and sum_a D_a^T (inv^T r)_a scattered onto y0 == ref_y_stiffness: the sign of
    det, the point order and the direction convention of r = w |det| inv(J_) grad_xi u are the reference's."""
    d = np.load(path)
    assert len(ANCHORS) >= 10
    inv, wdet, det = gc.point_factors(d["x_dofs"], d["x_g"], d["pts"], d["wts"])
    scale = np.max(np.abs(d["ref_detJ"]))
    assert np.max(np.abs(wdet - d["ref_detJ"])) <= 1e-13 * scale
    G = wdet[..., None, None] * np.einsum("cqda,cqdb->cqab", inv, inv)
    tri = np.stack([G[..., 0, 0], G[..., 0, 1], G[..., 0, 2], G[..., 1, 1], G[..., 1, 2], G[..., 2, 2]], axis=-1)
    assert np.max(np.abs(tri - d["ref_G"])) <= 1e-13 * np.max(np.abs(d["ref_G"]))

    dm, n = d["dofmap"], int(d["P"]) + 1
    r = gc.weighted_gradient(d["x_dofs"], d["x_g"], d["pts"], d["wts"], d["dphi_1d"], dm, d["x"])
    f = np.einsum("cqda,cqd->cqa", inv, r).reshape(-1, n, n, n, 3)  # (inv^T r)_a = G grad_xi u
    D = d["dphi_1d"].reshape(n, n)
    ye = (np.einsum("qi,cqjk->cijk", D, f[..., 0]) + np.einsum("qj,ciqk->cijk", D, f[..., 1]) + np.einsum("qk,cijq->cijk", D, f[..., 2]))
    y = d["y0"].copy()
    np.add.at(y, dm.reshape(-1), (d["cell_constants"][:, None] * ye.reshape(dm.shape[0], -1)).reshape(-1))
    tol = TOL[np.dtype(np.float64)]
    assert rel_l2(y, d["ref_y_stiffness"]) <= tol["l2"] and rel_max(y, d["ref_y_stiffness"]) <= tol["mx"]


# ---- 2. closed forms -------------------------------------------------------------------------------------------------------
def _geo(P, shape, perturb):
    mesh = pkg("boxmesh").BoxMesh(P, shape, perturb=perturb, seed=3)
    pts, wts, D = pkg("gll").tabulate_1d(P)
    return mesh, gc.Geometry.of_mesh(mesh, pts, wts, D)


@pytest.mark.parametrize("P", [1, 2, 4, 7])
def test_recovered_gradient_of_a_linear_field_is_its_slope(P):
    """A trilinear map carries a linear function exactly: C(1) u / M(1) 1 == a at EVERY dof of a perturbed mesh."""
    mesh, geo = _geo(P, (3, 2, 2), 0.15)
    a = np.array([1.3, -0.7, 2.1])
    u = mesh.dof_coordinates() @ a + 0.4
    g = gc.recovered_gradient(geo, u)
    assert np.max(np.abs(g - a[:, None])) <= 1e-11 * np.linalg.norm(a)
    cc = 1.0 + 0.5 * np.random.default_rng(2).random(mesh.ncells)  # with a constant per cell: the lumped-mass mean of c a
    gcst = gc.recovered_gradient(geo, u, cc)
    assert np.max(np.abs(gcst - a[:, None] * (geo.mass(cc) / geo.vol)[None, :])) <= 1e-11 * np.linalg.norm(a)


def test_intensity_of_a_linear_real_part_and_constant_imaginary_part():
    """Re P = alpha . x, Im P = beta: I = beta alpha / (2 k w rho) exactly -- fixes sign and factor."""
    mesh, geo = _geo(3, (3, 2, 2), 0.15)
    alpha, beta, k, omega, rho = np.array([2.0, -1.0, 0.5]), 3.0, 2, 2 * np.pi * 1.1e6, 1050.0
    re, im = mesh.dof_coordinates() @ alpha, np.full(mesh.ndofs, beta)
    I = gc.intensity_of(geo, k, omega, re, im, np.full(mesh.ncells, rho))
    expect = beta * alpha / (2 * k * omega * rho)
    assert np.max(np.abs(I - expect[:, None])) <= 1e-11 * np.linalg.norm(expect)
    vre, vim = gc.particle_velocity(geo, k, omega, re, im, np.full(mesh.ncells, rho))
    assert np.max(np.abs(vre)) <= 1e-11 * np.linalg.norm(alpha) / (k * omega * rho)
    assert np.max(np.abs(vim - (alpha / (k * omega * rho))[:, None])) <= 1e-11 * np.linalg.norm(alpha) / (k * omega * rho)


def test_a_plane_wave_towards_plus_x_carries_intensity_towards_plus_x():
    """p(t) = Re(P e^{i w t}) with P = e^{-i kappa x} travels towards +x: I_x > 0 (and close to 1 / (2 rho c)) at interior dofs."""
    mesh, geo = _geo(4, (4, 2, 2), 0.0)
    x = mesh.dof_coordinates()
    rho, c, omega = 1000.0, 1500.0, 2 * np.pi * 1500.0  # one wavelength over the unit box
    kappa = omega / c
    I = gc.intensity_of(geo, 1, omega, np.cos(kappa * x[:, 0]), -np.sin(kappa * x[:, 0]), np.full(mesh.ncells, rho))
    lo, hi = x.min(axis=0), x.max(axis=0)
    interior = np.all((x > lo + 1e-9) & (x < hi - 1e-9), axis=1)
    assert interior.sum() > 100 and np.all(I[0, interior] > 0.0)
    assert abs(np.median(I[0, interior]) * 2 * rho * c - 1.0) < 0.05
    assert np.max(np.abs(I[1:, interior])) < 1e-9 * np.max(I[0])


def test_radiation_force_of_a_uniform_medium_is_two_alpha_over_c_times_the_intensity():
    mesh, geo = _geo(2, (3, 2, 2), 0.1)
    x = mesh.dof_coordinates()
    k, omega, rho, c, delta = 1, 2 * np.pi * 1.0e6, 1000.0, 1500.0, 4.0e-6
    re, im = np.cos(3 * x[:, 0]) * (1 + x[:, 1]), np.sin(2 * x[:, 2])
    full = lambda v: np.full(mesh.ncells, v)  # noqa: E731
    F = gc.radiation_force(geo, [(k, omega, re, im)], full(delta), full(rho), full(c))
    I = gc.intensity_of(geo, k, omega, re, im, full(rho))
    assert rel_l2(F, delta * omega**2 / c**4 * I) <= 1e-13


# ---- 3. header, binding, validation ----------------------------------------------------------------------------------------
NAMES = ("fus_gradient_apply_planned_geom_f64", "fus_gradient_apply_planned_geom_f32")


def test_header_binding_and_library_carry_both_entry_points():
    lib_mod = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "fus_gpu.h")).read()
    raw = C.CDLL(lib_mod.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", hdr), name
        assert name in lib_mod.SIGNATURES and hasattr(raw, name)
        assert len(lib_mod.SIGNATURES[name]) == 13
    assert "GradientSpectral3D" in open(os.path.join(ROOT, "include", "fus_gpu.hpp")).read()
    assert lib_mod.load().fus_abi_version() == 3  # an addition: the ABI version stays


@pytest.mark.parametrize("name", NAMES)
def test_argument_validation_precedes_device_work(name):
    """Pointers that are never dereferenced (as tests/test_abi.py): every check fails, or passes, before any device work, in the
    order of the planned cell operators."""
    f = getattr(pkg("_lib").load(), name)
    z, one = C.c_void_p(0), C.c_void_p(256)
    ok = lambda y=one, ys=8, P=4, ncell=1, x=one, ws=one: f(x, one, y, ys, one, one, one, one, ws, one, P, ncell, z)  # noqa: E731
    assert ok(P=11) == -2 and ok(P=0) == -2
    assert ok(ncell=-1) == -1
    assert ok(y=z) == -1  # null y
    assert ok(ys=-1) == -1  # negative ystride
    assert ok(x=z) == -1 and ok(ws=z) == -1 and ok(ws=C.c_void_p(264)) == -1
    assert f(z, z, z, 0, z, z, z, z, z, z, 4, 0, z) == 0  # no cells: a no-op before any pointer is looked at
    assert ok(P=11, ncell=-1) == -1 and ok(P=11, ncell=0) == -2 and ok(y=z, P=11) == -2  # the order of planned_cell_entry
    assert ok() == -6  # all arguments well-formed, but no plan was built at this address: still no launch


def test_operator_constructor_errors():
    ops = pkg("operators")
    D = np.zeros(25)
    with pytest.raises(ValueError, match="geometry"):
        ops.gradient_operator(4, D, np.float64)
    with pytest.raises(ValueError, match="geometry"):
        ops.gradient_operator(4, D, np.float64, geometry=(None, None, None))
    with pytest.raises(ValueError, match="dphi"):
        ops.gradient_operator(4, None, np.float64, geometry=(None,) * 4)
    for P in (0, 11):
        with pytest.raises(ValueError, match="degree"):
            ops.gradient_operator(P, D, np.float64, geometry=(None,) * 4)


def test_map_argument_errors():
    import torch

    it, lib_mod = pkg("intensity"), pkg("_lib")
    mesh = types.SimpleNamespace(ncells=4)
    solver = types.SimpleNamespace(nlocal=10, ndofs=12, mesh=mesh, rho_cells=np.full(4, 1000.0), c_cells=np.full(4, 1500.0))
    host = torch.zeros(10, dtype=torch.float64)
    with pytest.raises(TypeError):
        it.recovered_gradient(solver, np.zeros(10))
    with pytest.raises(ValueError, match="owned dofs"):
        it.recovered_gradient(solver, torch.zeros(11, dtype=torch.float64))
    with pytest.raises(lib_mod.FusGpuError):
        it.recovered_gradient(solver, host)  # no CPU path
    with pytest.raises(ValueError, match="harmonic number"):
        it.intensity_of(solver, 0, 1.0, host, host)
    with pytest.raises(ValueError, match="omega"):
        it.intensity_of(solver, 1, 0.0, host, host)
    with pytest.raises(lib_mod.FusGpuError):
        it.intensity_of(solver, 1, 1.0, host, host)
    with pytest.raises(ValueError, match="rho_cells"):
        it.intensity_of(types.SimpleNamespace(nlocal=10, ndofs=12, mesh=mesh), 1, 1.0, host, host)
    monitor = types.SimpleNamespace(harmonics=(1, 2), omega=1.0, nacc=4)
    with pytest.raises(ValueError, match="not accumulated"):
        it.intensity(monitor, solver, harmonics=(3,))
    with pytest.raises(ValueError, match="no harmonics"):
        it.intensity(types.SimpleNamespace(harmonics=(), omega=None, nacc=4), solver)
    with pytest.raises(ValueError, match="delta_cells"):
        it.radiation_force(monitor, solver)  # the error heat_deposition raises for such a solver
    fm = pkg("field_monitor")
    assert callable(fm.FieldMonitor.intensity) and callable(fm.FieldMonitor.radiation_force)


# ---- 4. resource usage -----------------------------------------------------------------------------------------------------
# (T, P): (most VGPRs over the four (ORDERED, RUNS) shapes, LDS bytes per workgroup, waves per SIMD) of gradient_plan_geom_kernel as
# built; the fp64 P = 4 and P = 6 rows are quoted in DESIGN 3.10
PINNED = {
    ("double", 1): (90, 28776, 5), ("double", 2): (93, 32624, 5), ("double", 3): (102, 37096, 4), ("double", 4): (124, 23104, 4),
    ("double", 5): (120, 51048, 3), ("double", 6): (154, 29616, 3), ("double", 7): (164, 34472, 3), ("double", 8): (148, 71936, 2),
    ("double", 9): (148, 65512, 2), ("double", 10): (193, 44608, 2),
    ("float", 1): (57, 12352, 8), ("float", 2): (60, 13296, 8), ("float", 3): (63, 14472, 8), ("float", 4): (69, 16568, 7),
    ("float", 5): (111, 19488, 4), ("float", 6): (85, 21680, 5), ("float", 7): (94, 25448, 5), ("float", 8): (104, 27240, 4),
    ("float", 9): (102, 24768, 4), ("float", 10): (115, 32960, 4),
}

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


@pytest.fixture(scope="module")
def table():
    import resource_usage as ru

    return ru.parse(ru.cached_remarks())


def _rows(table, kernel, T, P):
    return [v for k, v in table.items() if re.search(rf"fus::{kernel}<{T}, {P}, ", k)]


@needs_hipcc
def test_every_instantiation_without_scratch(table):
    rows = [(k, v) for k, v in table.items() if "gradient_plan_geom_kernel<" in k]
    assert len(rows) == 2 * 10 * 4, len(rows)  # fp64 and fp32, degrees 1 .. 10, the four (ORDERED, RUNS) shapes
    assert not [(k, v["scratch"]) for k, v in rows if v["scratch"] != 0 or v["agpr"] != 0]


@needs_hipcc
@pytest.mark.parametrize("T,P", sorted(PINNED), ids=[f"{t}-P{p}" for t, p in sorted(PINNED)])
def test_registers_lds_and_occupancy_as_built(table, T, P):
    vgpr, lds, occ = PINNED[(T, P)]
    rows = _rows(table, "gradient_plan_geom_kernel", T, P)
    assert len(rows) == 4
    assert max(r["vgpr"] for r in rows) == vgpr and {r["lds"] for r in rows} == {lds} and {r["occupancy"] for r in rows} == {occ}, rows
    # never fewer waves per SIMD than the stiffness apply with in-kernel geometry of the same scalar type and degree
    assert occ >= min(r["occupancy"] for r in _rows(table, "stiffness_plan_geom_kernel", T, P))


@needs_hipcc
def test_pinned_table_is_complete():
    assert sorted(PINNED) == sorted((T, P) for T in ("double", "float") for P in range(1, 11))
