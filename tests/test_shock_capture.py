"""Shock capturing without a GPU: the header and its binding, the build lists, the modal table, the exact cases of the CPU model
(tests/shock_model.py), the resource pins of every shipped build of csrc/modal_sensor.hpp and the refusals of the binding."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest
import shock_model as sm
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fus_gpu_sensor.h")
ENTRY_POINTS = ("fus_modal_sensor_f64", "fus_modal_sensor_f32")
DEGREES = range(1, 11)  # every degree the Westervelt cell operator ships for

# Occupancy [waves/SIMD] the compiler reports for modal_sensor_kernel<T, P, default_cells_per_block(P, 256)>, by degree
OCCUPANCY = {"double": {1: 8, 2: 8, 3: 8, 4: 7, 5: 6, 6: 5, 7: 4, 8: 4, 9: 4, 10: 3},
             "float": {1: 8, 2: 8, 3: 8, 4: 8, 5: 8, 6: 8, 7: 8, 8: 8, 9: 8, 10: 7}}


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_parsed_into_the_open_tier():
    lib_mod = pkg("_lib")
    assert HEADER in lib_mod.LATER_HEADER_PATHS
    assert lib_mod.LATER_HEADER_PATHS[-1].endswith("fus_gpu_waveform.h")  # tests/test_waveform_sources.py pins it as the last
    functions, defines = lib_mod.parse_header(read(HEADER))
    assert tuple(functions) == ENTRY_POINTS and defines == {"FUS_SENSOR_QUIET": -1000}
    assert sm.QUIET == defines["FUS_SENSOR_QUIET"] == pkg("shock_capture").QUIET
    ptr, dbl = C.c_void_p, C.c_double
    for name in ENTRY_POINTS:
        assert lib_mod.LATER[name] == (C.c_int, [ptr] * 9 + [C.c_int, C.c_int64, dbl, dbl, dbl, dbl, ptr])
        assert name not in lib_mod.DECLARATIONS and name not in lib_mod.EXTENSIONS and name not in lib_mod.ADDITIONS
    assert lib_mod.ABI_VERSION == 3
    assert '#include "fus_gpu_sensor.h"' in read(ROOT, "include", "fus_gpu.hpp") and '#include "fus_gpu.h"' in read(HEADER)


def test_library_exports_the_entry_points():
    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        assert fn.argtypes == lib_mod.LATER[name][1] and fn.restype is lib_mod.LATER[name][0]
    assert lib.fus_abi_version() == 3


def test_argument_checks_launch_nothing():
    """Refusals come back before any device work: the pointers are never dereferenced (this runs without a GPU)."""
    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    z, p = C.c_void_p(0), C.c_void_p(4096)
    invalid, degree = -1, lib_mod._DEFINES["FUS_ERR_UNSUPPORTED_DEGREE"]
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)

        def call(ptrs=(p,) * 9, P=4, ncell=8, s0=-2.4, kappa=1.0, floor=1.0, hold=0.0):
            return fn(*ptrs, P, ncell, s0, kappa, floor, hold, z)

        assert call(ncell=-1) == invalid
        assert call(P=0) == degree and call(P=11) == degree and call(P=0, ncell=0) == degree
        for k in range(9):  # each of the nine pointers
            assert call(ptrs=tuple(z if i == k else p for i in range(9))) == invalid, k
        assert call(kappa=0.0) == invalid and call(kappa=float("nan")) == invalid and call(floor=-1.0) == invalid
        assert call(hold=1.5) == invalid and call(hold=-0.1) == invalid and call(s0=float("nan")) == invalid
        for P in DEGREES:
            assert call(ptrs=(z,) * 9, P=P, ncell=0) == 0  # the empty mesh: nothing launched, no pointer looked at


def test_build_lists():
    mk = read(CSRC, "Makefile")
    src = re.search(r"^SRC = (.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR = (.*)$", mk, re.M).group(1).split()
    obj = re.search(r"^OBJ = (.*)$", mk, re.M).group(1).split()
    assert "abi_sensor.hip" in src and "_obj/abi_sensor.o" in obj
    assert "modal_sensor.hpp" in hdr and "../../include/fus_gpu_sensor.h" in hdr  # the source hash covers them
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage

    assert all(unit != "abi_sensor.hip" for unit, _ in resource_usage.UNITS)
    for tool in ("resource_usage.py", "compare_kernels.py"):
        assert '"fus_gpu_sensor.h"' in read(ROOT, "tools", tool), tool
    # no unit that the kernel census compiles includes the sensor kernel, and the new files stay out of tests/test_reduce.py's scan
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".hpp")) and name not in ("abi_sensor.hip", "modal_sensor.hpp"):
            assert "modal_sensor.hpp" not in read(CSRC, name), name
    for name in ("abi_sensor.hip", "modal_sensor.hpp"):
        assert "reduce.hpp" not in read(CSRC, name)
    assert "atomic" not in re.sub(r"//[^\n]*", "", read(CSRC, "modal_sensor.hpp")).lower()  # a fixed order: no atomics in the code


@pytest.mark.parametrize("P", range(2, 11))
def test_modal_table_is_the_inverse(P):
    """Vinv V = I to 1e-13, V rebuilt here by ``legval``; V^T W is NOT the inverse (the GLL rule does not integrate P_P^2)."""
    sc, gll = pkg("shock_capture"), pkg("gll")
    V, Vinv = sm.vandermonde(P), sc.modal_table(P)
    assert np.max(np.abs(V - sc.vandermonde(P))) <= 1e-13
    assert np.max(np.abs(Vinv @ V - np.eye(P + 1))) <= 1e-13
    assert np.max(np.abs(Vinv - sm.table(P))) <= 1e-13
    w = 2.0 * gll.tabulate_1d(P)[1]  # weights on [-1, 1]
    assert np.max(np.abs((V.T * w) @ V - np.eye(P + 1))) > 0.1  # the last diagonal entry is (2 P + 1) / P


def _one_cell(P, f):
    """``f(xi_x, xi_y, xi_z)`` at the nodes of one reference cell, as a field with the identity dofmap."""
    xi = 2.0 * pkg("gll").tabulate_1d(P)[0] - 1.0
    X, Y, Z = np.meshgrid(xi, xi, xi, indexing="ij")
    n3 = (P + 1) ** 3
    return f(X, Y, Z).reshape(-1), np.arange(n3, dtype=np.int32).reshape(1, n3)


@pytest.mark.parametrize("P", range(2, 9))
def test_model_exact_cases(P):
    leg = np.polynomial.legendre.Legendre
    s0, kappa, eps_max = float(pkg("shock_capture").default_s0(P)), 0.5, np.array([0.37])
    # a polynomial of degree <= P - 1 per axis: no top-mode energy but what the transform's cancellation leaves
    u, dm = _one_cell(P, lambda x, y, z: (1.0 + x) ** (P - 1) * (2.0 - y) ** (P - 1) + 3.0 * z ** (P - 1) - x * y * z)
    out = sm.sensor(u, dm, P, 1e-6, s0, kappa, eps_max)
    print(f"P={P}: smooth top {out['top'][0]:.3e} (bound {out['btop'][0]:.3e}), tot {out['tot'][0]:.3e}")
    assert out["top"][0] <= out["btop"][0] and out["tot"][0] > 1.0 and out["eps"][0] == 0.0
    # tot is the integral of u^2 over the reference cell (the modes are orthonormal): a constant c gives 8 c^2
    u, dm = _one_cell(P, lambda x, y, z: 2.5 + 0.0 * x)
    assert abs(sm.sensor(u, dm, P, 1e-6, s0, kappa, eps_max)["tot"][0] - 8.0 * 2.5**2) <= 1e-12
    # the pure mode P_P(xi_x): all of its energy is top energy
    u, dm = _one_cell(P, lambda x, y, z: leg.basis(P)(x) + 0.0 * y)
    out = sm.sensor(u, dm, P, 1e-6, s0, kappa, eps_max)
    assert abs(out["top"][0] / out["tot"][0] - 1.0) <= 1e-13 and abs(out["s"][0]) <= 1e-13 and out["eps"][0] == eps_max[0]
    # a step inside the cell lies above the ramp
    u, dm = _one_cell(P, lambda x, y, z: np.where(x > 0.1, 1.0, -1.0) + 0.0 * y)
    out = sm.sensor(u, dm, P, 1e-6, s0, kappa, eps_max)
    print(f"P={P}: step s {out['s'][0]:.3f}, ramp top {s0 + kappa:.3f}")
    assert out["s"][0] >= s0 + kappa and out["r"][0] == 1.0 and out["eps"][0] == eps_max[0]
    # quiet: the same step below the floor; the hold keeps a share of the last value; cc4 is the base where eps == 0
    quiet = sm.sensor(u, dm, P, 2.0, s0, kappa, eps_max, eps_prev=np.array([0.2]), hold=0.5)
    assert quiet["s"][0] == sm.QUIET and quiet["r"][0] == 0.0 and quiet["eps"][0] == 0.1
    eps, cc4 = sm.update(np.array([0.0, 1.0]), np.array([0.3, 0.3]), np.zeros(2), 0.0, np.array([-1e-9, -1e-9]), np.array([4e-10, 4e-10]))
    assert eps.tolist() == [0.0, 0.3] and cc4[0] == -1e-9 and cc4[1] == -1e-9 - 0.3 * 4e-10
    # the ramp: 0, 1/2, 1 at its three marks, monotone in between
    marks = sm.ramp(np.array([s0 - kappa, s0, s0 + kappa]), s0, kappa)
    assert marks.tolist() == [0.0, 0.5, 1.0] and np.all(np.diff(sm.ramp(np.linspace(s0 - 2, s0 + 2, 101), s0, kappa)) >= 0.0)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_sensor_kernels_resource_pin():
    """Exactly the shipped builds -- 10 degrees x 2 types at default_cells_per_block(P, 256) cells per workgroup -- each without scratch
    and without AGPRs, with no more LDS than the three cubes of stiffness_col_kernel at the same degree, at the occupancy the
    compiler reports."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage

    table = resource_usage.parse(resource_usage.compile_remarks("abi_sensor.hip"))
    got = {}
    for name, d in table.items():
        m = re.match(r"(?:void )?fus::modal_sensor_kernel<(double|float), (\d+), (\d+)>\(", name)
        assert m, f"a kernel that is not the sensor kernel in abi_sensor.hip: {name}"
        got[(m[1], int(m[2]), int(m[3]))] = d
    assert set(got) == {(t, P, max(256 // (P + 1) ** 2, 1)) for t in ("double", "float") for P in DEGREES}
    for (t, P, cpb), d in got.items():
        n, size = P + 1, 8 if t == "double" else 4
        stride = n**3
        while stride % 32 != (8 if P < 8 else 16):  # lds_cell_stride (csrc/stiffness.hpp)
            stride += 1
        cube = cpb * stride * size
        assert d["scratch"] == 0 and d["agpr"] == 0, (t, P, d)
        assert d["lds"] == 2 * cube + n * n * size and d["lds"] <= 3 * cube, (t, P, d)
        assert d["occupancy"] == OCCUPANCY[t][P], (t, P, d)


def test_binding_refusals():
    """The two combinations out of scope raise before any device work; so do parameters outside their ranges."""
    sc, nl, nm = pkg("shock_capture"), pkg("nonlinear_solver"), pkg("nodal_medium")
    mesh = sm.thin_box(2, 0.002, P=2)
    with pytest.raises(ValueError, match="uniform_ratio=True"):
        nl.WesterveltSpectral3D(mesh, fused=True, uniform_ratio=True, shock_capture=sc.ShockCapture())
    medium = nm.NodalMedium(np.full(mesh.ndofs, 1500.0), np.full(mesh.ndofs, 1000.0))
    with pytest.raises(ValueError, match="out of scope"):
        nl.WesterveltSpectral3D(mesh, fused=True, nodal_medium=medium, shock_capture=sc.ShockCapture())
    for bad in (dict(strength=-1.0), dict(kappa=0.0), dict(hold=1.5), dict(every=0), dict(floor=-1.0)):
        with pytest.raises(ValueError):
            sc.ShockCapture(**bad)
    cap = sc.ShockCapture()
    assert (cap.strength, cap.kappa, cap.hold, cap.every, cap.s0, cap.floor) == (0.1, 0.5, 0.0, 1, None, None)
    with pytest.raises(pkg("_lib").FusGpuError, match="not bound"):
        cap.artificial_diffusivity()


def test_solver_cases_on_the_cpu_model():
    """The condition the high-drive case was chosen by, on the CPU model of the run: the plain overshoot is at least twice the
    captured one and both runs stay finite; and the low-drive case never leaves the ramp's foot.  The recorded values are what the
    GPU test's midpoint comes from."""
    case = sm.HIGH_DRIVE
    mesh = sm.thin_box(case["ncells"], case["length"])
    h = case["length"] / case["ncells"]
    per_period = int(1.0 / sm.F0 / (0.4 * h / (sm.C0 * mesh.P**2))) + 1
    assert case["dt"] == 1.0 / sm.F0 / per_period and case["steps"] == 12 * per_period
    assert sm.shock_distance(case["p0"]) < 0.5 * case["length"]
    over = {}
    for name, capture in (("plain", None), ("captured", sm.default_capture(mesh, case["p0"]))):
        run = sm.Run(mesh, case["p0"], sm.ATT_DB, capture)
        u, v = run.advance(case["steps"], case["dt"])
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(v))
        over[name] = run.peak / case["p0"] - 1.0
        if capture is not None:
            assert (run.eps > 0).sum() > mesh.ncells // 2 and run.eps.max() <= capture["eps_max"].max()
    print("CPU model overshoot:", over)
    assert over["plain"] >= 2.0 * over["captured"]
    for name in over:
        assert abs(over[name] - case[f"overshoot_{name}"]) <= 1e-9 * over[name]
    low = sm.LOW_DRIVE
    mesh = sm.thin_box(low["ncells"], low["length"])
    capture = sm.default_capture(mesh, low["p0"])
    run = sm.Run(mesh, low["p0"], sm.ATT_DB, capture)
    worst = sm.QUIET
    for _ in range(6):
        run.advance(low["steps"] // 6, low["dt"])
        assert np.all(run.eps == 0.0)
        worst = max(worst, run.sensor.max())
    print("low drive: largest sensor value at the six checks", worst, "ramp foot", capture["s0"] - capture["kappa"])
    assert sm.QUIET < worst < capture["s0"] - capture["kappa"] and run.max_eps == 0.0
