"""Power-law absorption through relaxation mechanisms, without a GPU: the fit, the frequency-domain formulas, the CPU model
(tests/relaxation_cpu.py) against the oracle's loops and against the theory on a plane wave, the guards, the HIP-free kinds table
on the host, and the kernel's resource usage."""

import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import relaxation_cpu
from conftest import ROOT, pkg
from oracle import rk4_oracle


# ---- the fit and the formulas ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y", [1.1, 1.3, 1.5])
def test_fit_power_law(y):
    """alpha0 = 0.5 dB/cm/MHz^y, c = 1540, 0.5-5 MHz, two mechanisms and the thermoviscous term: largest relative error <= 0.05
    (measured: 0.034, 0.044, 0.036 for y = 1.1, 1.3, 1.5), every weight non-negative, and the returned error is that of the model."""
    rx = pkg("relaxation")
    fit = rx.fit_power_law(0.5, y, 0.5e6, 5e6, n=2, speed_of_sound=1540.0, with_thermoviscous=True)
    print(f"y = {y}: kappa {fit.kappa}, delta {fit.delta:.3e}, largest relative error {fit.max_rel_error:.4f}")
    assert fit.max_rel_error <= 0.05
    assert fit.tau.shape == (2,) and np.all(fit.kappa >= 0.0) and fit.delta >= 0.0 and fit.kappa.sum() > 0.0
    assert np.allclose(1.0 / (2 * np.pi * fit.tau), [0.5e6, 5e6], rtol=1e-12)  # relaxation frequencies log-spaced from f_lo to f_hi
    f = np.geomspace(0.5e6, 5e6, 64)
    model = rx.RelaxationAbsorption(fit.tau, fit.kappa)
    alpha = model.alpha(f, 1540.0) + fit.delta * (2 * np.pi * f) ** 2 / (2 * 1540.0**3)
    target = 0.5 * np.log(10) / 20 * 100 * (f / 1e6) ** y
    assert abs(np.max(np.abs(alpha / target - 1.0)) - fit.max_rel_error) < 1e-12
    # the same times for another tissue: per-tissue weights share tau
    other = rx.fit_power_law(0.75, y, 0.5e6, 5e6, speed_of_sound=1540.0, tau=fit.tau)
    assert np.array_equal(other.tau, fit.tau) and np.allclose(other.kappa, 1.5 * fit.kappa, rtol=1e-8)


def test_alpha_and_phase_speed_are_first_order_in_kappa():
    """``alpha()`` and ``phase_speed()`` against the complex k(w) = (w / c)(1 + S)^(-1/2): the differences are second order in kappa --
    they fall by 4 when every weight is halved -- and of the size of kappa^2."""
    rx = pkg("relaxation")
    c, f = 1540.0, np.geomspace(0.3e6, 6e6, 23)
    tau = 1.0 / (2 * np.pi * np.array([0.5e6, 5e6]))
    errs = []
    for s in (1.0, 0.5, 0.25):
        m = rx.RelaxationAbsorption(tau, s * np.array([0.012, 0.02]))
        k = m.wavenumber(f, c)
        ea = np.abs(m.alpha(f, c) - (-k.imag)) / (-k.imag)  # relative: first order in kappa
        ec = np.abs(m.phase_speed(f, c) - 2 * np.pi * f / k.real) / c  # relative: second order in kappa
        errs.append((ea, ec))
        assert np.all(ea < 2.0 * s * 0.032) and np.all(ec < (s * 0.032) ** 2)
    for (ea1, ec1), (ea2, ec2) in zip(errs, errs[1:]):
        assert np.all((ea1 / ea2 > 1.9) & (ea1 / ea2 < 2.1))  # relative error of alpha ~ kappa: absolute error ~ kappa^2
        # (the second-order coefficient of the speed changes sign inside the band: its largest value, not each frequency's)
        assert 3.7 < ec1.max() / ec2.max() < 4.3
    m = rx.RelaxationAbsorption(tau, [0.012, 0.02])
    assert m.phase_speed(1.0, c) - c < 1e-9 * c  # speed_of_sound is the low-frequency limit


def test_model_argument_checks():
    rx = pkg("relaxation")
    for tau, kappa in (([1e-7] * 5, [0.1] * 5), ([1e-7, -1e-7], [0.1, 0.1]), ([1e-7], [-0.1]), ([1e-7, 1e-8], [0.1]), ([], [])):
        with pytest.raises(ValueError):
            rx.RelaxationAbsorption(tau, kappa)
    m = rx.RelaxationAbsorption([1e-7, 1e-8], np.full((2, 5), 0.01))
    assert not m.homogeneous and m.nr == 2


# ---- the CPU model -----------------------------------------------------------------------------------------------------------------
def _small_mesh(P=2):
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    mesh = boxmesh.BoxMesh(P, (2, 2, 2), length=0.006, perturb=0.1, seed=5)
    h = ls.time_step_parameters(mesh, P, 1500.0, 0.5e6, 0.006)
    return mesh, ls.snap_time_step(h, P, 1500.0, 0.5e6, 0.006)[0]


@pytest.mark.parametrize("which", ["linear", "westervelt"])
def test_cpu_model_without_weights_is_the_oracle(which):
    """Every kappa == 0: the restated loop over (u, v, xi) gives the fields of rk4_oracle.solve / solve_westervelt bit for bit, and xi
    stays zero; with weights the fields move."""
    mesh, dt = _small_mesh()
    tau, zero = np.array([3e-7, 3e-8]), np.zeros(2)
    if which == "linear":
        ref = rk4_oracle.solve(mesh, 6, dt)
        got = relaxation_cpu.solve(mesh, 6, dt, tau, zero)
        lossy = relaxation_cpu.solve(mesh, 6, dt, tau, np.array([0.05, 0.05]))
    else:
        kw = dict(c0=1500.0, f0=0.5e6)
        ref = rk4_oracle.solve_westervelt(mesh, 6, dt, **kw)
        got = relaxation_cpu.solve_westervelt(mesh, 6, dt, tau, zero, **kw)
        lossy = relaxation_cpu.solve_westervelt(mesh, 6, dt, tau, np.array([0.05, 0.05]), **kw)
    assert np.max(np.abs(ref[0])) > 0
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not np.any(got[2])
    assert np.max(np.abs(lossy[0] - ref[0])) > 1e-6 * np.max(np.abs(ref[0])) and np.any(lossy[2])


def test_cpu_model_per_cell_weights_are_the_lumped_average():
    """Weights that jump between cells: the per-dof weight is M(kappa) 1 / M(1) 1 -- the cell's value inside a cell, between the
    neighbours' values on a shared dof; equal weights in every cell are the scalar form."""
    mesh, _ = _small_mesh()
    detJ = rk4_oracle.host_detJ(mesh)
    from oracle import oracle_np

    kc = np.stack([np.linspace(0.01, 0.08, mesh.ncells), np.full(mesh.ncells, 0.03)])
    kd = relaxation_cpu.dof_weights(mesh, detJ, kc, oracle_np.mass_apply)
    assert np.allclose(kd[1], 0.03, rtol=1e-13)
    counts = np.bincount(mesh.dofmap.ravel(), minlength=mesh.ndofs)
    for c in range(mesh.ncells):
        inner = mesh.dofmap[c][counts[mesh.dofmap[c]] == 1]
        assert inner.size and np.allclose(kd[0, inner], kc[0, c], rtol=1e-13)
    assert np.all(kd[0] >= kc[0].min() - 1e-15) and np.all(kd[0] <= kc[0].max() + 1e-15)


def test_cpu_model_plane_wave_absorbs_and_disperses_as_the_theory(oracle_c):
    """A continuous plane wave along a row of 60 cubic P = 4 cells (3 per wavelength, 20 wavelengths, rigid lateral walls), linear
    model, two mechanisms with homogeneous weights, 30 periods; the fundamental over the last period, fitted between 1 and 19
    wavelengths (the amplitude falls by e^-0.6 there): the slope of its log-amplitude against alpha_r(w0), the slope of its phase
    against c_ph(w0).  Measured with this model on this mesh: alpha 2.02 % below the first-order alpha_r (1.2e-5 from the exact
    -Im k: the deviation IS the second-order term, 3/2 Re S), speed 1.27e-5 above c_ph.  The bounds are twice that: 4.05 % and
    2.6e-5 (the conditions: at most 5 % and 0.1 %)."""
    k = relaxation_cpu.plane_wave_case()
    model, w0 = k["model"], 2 * np.pi * k["f0"]
    model.check_time_step(k["dt"])
    acc = np.zeros(k["mesh"].ndofs, dtype=complex)
    t_from = (k["periods"] - 1) / k["f0"] + 0.5 * k["dt"]

    def record(t, u, v):
        if t > t_from:
            acc[:] += u * np.exp(-1j * w0 * t)

    relaxation_cpu.solve(k["mesh"], k["per"] * k["periods"], k["dt"], model.tau, model.kappa, c0=k["c"], f0=k["f0"], oracle_c=oracle_c,
                         record=record)
    x = k["mesh"].dof_coordinates()[:, 0]
    amp = np.abs(acc) * 2 / k["per"]
    alpha, kx = relaxation_cpu.fit_slopes(x, amp, np.angle(acc), *k["x_fit"])
    alpha_r, c_ph = model.alpha(k["f0"], k["c"]), model.phase_speed(k["f0"], k["c"])
    da, dc = alpha / alpha_r - 1.0, (w0 / kx) / c_ph - 1.0
    print(f"plane wave, CPU model: alpha {alpha:.5f} against {alpha_r:.5f} ({da:+.3e}), speed {w0 / kx:.4f} against {c_ph:.4f} ({dc:+.3e})")
    assert alpha_r * (k["x_fit"][1] - k["x_fit"][0]) >= 0.5 and c_ph - k["c"] > 5.0  # the loss and the dispersion are there to be seen
    assert abs(da) <= PLANE_WAVE_ALPHA_BOUND and abs(dc) <= PLANE_WAVE_SPEED_BOUND


# twice what the CPU model shows on the mesh of relaxation_cpu.plane_wave_case (the docstring above); tests/test_relaxation_gpu.py uses them
PLANE_WAVE_ALPHA_BOUND = 2 * 0.02024
PLANE_WAVE_SPEED_BOUND = 2 * 1.27e-5
assert PLANE_WAVE_ALPHA_BOUND <= 0.05 and PLANE_WAVE_SPEED_BOUND <= 1e-3


# ---- the guards --------------------------------------------------------------------------------------------------------------------
def test_time_step_guard():
    """dt / min(tau) >= 2.785 (the real-axis stability limit of the classical RK4) is refused; just below it is not."""
    rx = pkg("relaxation")
    m = rx.RelaxationAbsorption([1e-6, 1e-7], [0.01, 0.01])
    m.check_time_step(2.78e-7)
    for dt in (2.785e-7, 1e-6):
        with pytest.raises(ValueError, match="2.785"):
            m.check_time_step(dt)


def test_uniform_ratio_with_relaxation_is_refused():
    """The single-gather form w = u_n + kappa v_n is out of scope: refused before any device work."""
    rx, nls, boxmesh = pkg("relaxation"), pkg("nonlinear_solver"), pkg("boxmesh")
    mesh = boxmesh.BoxMesh(2, (2, 2, 2), length=0.006)
    with pytest.raises(ValueError, match="uniform_ratio"):
        nls.WesterveltSpectral3D(mesh, np.float64, uniform_ratio=True, relaxation=rx.RelaxationAbsorption([1e-7], [0.01]))


# ---- the kinds table on the host, the kernel's resources ---------------------------------------------------------------------------
def test_relax_table_host_program(tmp_path):
    """csrc/relax_table.hpp on its own: tests/host/relax_table_check.cpp, built with the host compiler (no HIP, no GPU) and run."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "relax_table_check")
    src = os.path.join(ROOT, "tests", "host", "relax_table_check.cpp")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RELAX_TABLE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_relax_stage_kernel_resources():
    """Every instantiation (2 types x NR 1..4 x wide / scalar x 3 streaming policies x per-dof / scalar weights = 96): no scratch, no
    LDS, eight waves per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    table = {k: v for k, v in ru.parse(ru.cached_remarks()).items() if re.search(ru.ALIASES["relaxation"], k)}
    assert len(table) == 96, sorted(table)
    for name, d in table.items():
        assert d["scratch"] == 0 and d["lds"] == 0 and d["agpr"] == 0 and d["occupancy"] >= 8 and d["vgpr"] <= 64, (name, d)


def test_binding_declares_the_entry_points():
    """fus_relax_stage_* come from include/fus_gpu_relaxation.h through the header parser, with the header's types (include/fus_gpu.h
    and fus_gpu_array.h keep their pinned sets of functions: ``_lib.ADDITIONS`` holds what later headers declare), the library exports
    them, include/fus_gpu.hpp includes the header, and the ABI version stays 3."""
    import ctypes as C

    lib_mod = pkg("_lib")
    d, f, i, i64, vp = C.c_double, C.c_float, C.c_int, C.c_int64, C.c_void_p
    assert lib_mod.ADDITIONS["fus_relax_stage_f64"] == (i, [d, d, d, i, i] + [vp] * 6 + [i64] + [vp] * 3 + [i64, vp])
    assert lib_mod.ADDITIONS["fus_relax_stage_f32"] == (i, [f, f, f, i, i] + [vp] * 6 + [i64] + [vp] * 3 + [i64, vp])
    assert set(lib_mod.ADDITIONS) == {"fus_relax_stage_f64", "fus_relax_stage_f32"}
    assert '#include "fus_gpu_relaxation.h"' in open(os.path.join(ROOT, "include", "fus_gpu.hpp")).read()
    lib = lib_mod.load()
    assert lib_mod.ABI_VERSION == 3 and lib.fus_abi_version() == 3 and list(lib.fus_relax_stage_f64.argtypes) == lib_mod.ADDITIONS["fus_relax_stage_f64"][1]
    z, one = C.c_void_p(0), C.c_void_p(256)
    tau = (C.c_double * 4)(1e-7, 1e-7, 1e-7, 1e-7)
    tp = C.cast(tau, C.c_void_p)
    call = lambda kind, nr, n, stride, p=one, t=tp: lib.fus_relax_stage_f64(1.0, 1.0, 1.0, kind, nr, t, t, z, p, p, p, stride, p, p, p, n, z)  # noqa: E731
    assert call(0, 2, 0, 0) == 0  # nothing to do
    assert call(3, 2, 4, 4) == -1 and call(0, 5, 4, 4) == -1 and call(0, 0, 4, 4) == -1 and call(0, 2, 4, 3) == -1 and call(0, 2, -1, 4) == -1
    assert call(0, 2, 4, 4, z) == -1 and call(0, 2, 4, 4, one, z) == -1  # a null array, null tau: before any device work
    tau[1] = 0.0
    assert call(0, 2, 4, 4) == -1
