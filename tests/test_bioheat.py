"""Pennes bioheat, the parts that need no GPU: the CPU restatement the GPU tests compare with (tests/bioheat_cpu.py) against
closed forms, the constructor's argument checks, the power gate, and the new symbol in the header and the binding."""

import math
import os
import re
import shutil
import sys

import numpy as np
import pytest

import bioheat_cpu as bc
from conftest import ROOT, pkg

RHO_C = 1050.0 * 3600.0


@pytest.fixture(scope="module")
def box():
    mesh = pkg("boxmesh").BoxMesh(2, (3, 2, 2), perturb=0.15)
    cpu = bc.CpuBioheat(mesh, 0.5, RHO_C)
    return mesh, cpu, cpu.lambda_max()


def test_cpu_loop_conserves_heat_and_adds_the_source(box):
    """K 1 = 0 and K symmetric: sum_d m_d T_d is constant without perfusion and source, and grows by dt sum_d vol_d q_d per step
    with a constant gate (RK4 integrates a constant exactly)."""
    mesh, _, lam = box
    cpu = bc.CpuBioheat(mesh, 0.5, RHO_C)
    dt = 0.8 * 2.785 / lam
    cpu.T = 37.0 + 8.0 * np.random.default_rng(1).random(mesh.ndofs)
    heat0 = math.fsum(cpu.mc * cpu.T)
    cpu.advance(0.0, 20 * dt, dt, max_steps=20)
    assert abs(math.fsum(cpu.mc * cpu.T) - heat0) <= 1e-13 * heat0
    q = 1e3 * bc.smooth_field(mesh, 3)
    cpu.set_heat_source(q)
    for _ in range(3):
        before = math.fsum(cpu.mc * cpu.T)
        cpu.advance(0.0, dt, dt)
        grown = math.fsum(cpu.mc * cpu.T) - before
        assert abs(grown - dt * math.fsum(cpu.vol * q)) <= 1e-13 * before


def test_cpu_loop_perfusion_decay_is_the_rk4_polynomial(box):
    mesh, _, lam = box
    pr = 0.2 * lam
    cpu = bc.CpuBioheat(mesh, 0.5, RHO_C, w=pr * RHO_C)
    dt, n = 0.8 * 2.785 / (lam + pr), 10
    cpu.T = np.full(mesh.ndofs, 42.0)
    cpu.advance(0.0, n * dt, dt, max_steps=n)
    expect = 37.0 + 5.0 * bc.rk4_growth(pr * dt) ** n
    assert np.max(np.abs(cpu.T - expect)) <= 64 * n * np.finfo(np.float64).eps * 42.0


@pytest.mark.parametrize("T,factor", [(45.0, 4.0), (41.0, 1.0 / 16.0), (43.0, 1.0)])
def test_cpu_loop_dose_of_a_uniform_field(box, T, factor):
    mesh, _, lam = box
    cpu = bc.CpuBioheat(mesh, 0.5, RHO_C)
    dt, n = 0.8 * 2.785 / lam, 7
    cpu.T = np.full(mesh.ndofs, T)
    cpu.advance(0.0, n * dt, dt, max_steps=n)
    tol = 64 * n * np.finfo(np.float64).eps * T
    assert np.max(np.abs(cpu.T - T)) <= tol and np.max(np.abs(cpu.tmax - T)) <= tol
    assert np.max(np.abs(cpu.cem43 / (n * dt / 60.0 * factor) - 1.0)) <= math.log(4.0) * tol + 4 * np.finfo(np.float64).eps


def test_cpu_loop_fixed_dofs_and_dense_operator(box):
    mesh, cpu0, lam = box
    fixed = np.unique(mesh.facet_dofmap(mesh.boundary_facets([3])))
    cpu = bc.CpuBioheat(mesh, 0.5, RHO_C, fixed=fixed)
    cpu.T = 37.0 + 8.0 * np.random.default_rng(2).random(mesh.ndofs)
    T0 = cpu.T.copy()
    dt = 0.8 * 2.785 / lam
    cpu.advance(0.0, 5 * dt, dt)
    assert np.array_equal(cpu.T[fixed], T0[fixed])
    free = np.setdiff1d(np.arange(mesh.ndofs), fixed)
    assert np.max(np.abs(cpu.T[free] - T0[free])) > 0.1
    ev = np.linalg.eigvals(cpu0.dense_minv_K()).real
    assert ev.min() > -1e-12 * ev.max() and 0.9 * ev.max() < lam <= ev.max() * (1 + 1e-12)  # the power iteration is a lower bound


def test_stage_reference_matches_the_loop(box):
    """The dof-wise stage the kernel test compares with, chained FIRST, MIDDLE, MIDDLE, LAST, is the loop's step."""
    mesh, _, lam = box
    pr = 0.1 * lam
    cpu = bc.CpuBioheat(mesh, 0.5, RHO_C, w=pr * RHO_C)
    cpu.set_heat_source(1e3 * bc.smooth_field(mesh, 4))
    cpu.T = 37.0 + 3.0 * bc.smooth_field(mesh, 5)
    dt = 0.5 / lam
    T0, Tn, acc, cem = cpu.T.copy(), np.zeros(mesh.ndofs), np.zeros(mesh.ndofs), np.zeros(mesh.ndofs)
    for i in range(4):
        b = -cpu.K(T0 if i == 0 else Tn)
        kind = 2 if i == 3 else (0 if i == 0 else 1)
        out, _ = bc.stage_reference(kind, bc.B[i] * dt, 0.0 if i == 3 else bc.A[i + 1] * dt, 1.0, 37.0, dt, cpu.minv, b, T0, Tn, acc,
                                    pr=cpu.pr, s=cpu.s, cem43=cem, init=True)
        if kind == 2:
            T0, cem = out["T0"], out["cem43"]
        else:
            acc, Tn = out["acc"], out["Tn"]
    cpu.advance(0.0, dt, dt)
    assert np.max(np.abs(T0 - cpu.T)) <= 1e-13 * 40 and np.max(np.abs(cem / cpu.cem43 - 1)) <= 1e-12


def test_power_gate():
    parse = pkg("bioheat").parse_power
    assert parse(None)(123.0) == 1.0
    g = parse((1.0, 2.5))
    assert [g(t) for t in (0.5, 1.0, 2.0, 2.5, 3.0)] == [0.0, 1.0, 1.0, 0.0, 0.0]
    assert parse((0.0, 0.0))(0.0) == 0.0  # an empty window: cooling
    pulsed = parse(lambda t: 0.25 if int(t) % 2 == 0 else 0)
    assert pulsed(0.5) == 0.25 and pulsed(1.5) == 0.0 and isinstance(pulsed(1.5), float)
    for bad in ((2.0, 1.0), (1.0,), 3.0, "on", (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            parse(bad)


def test_constructor_argument_errors():
    """Checked before any device work: these raise on a machine without a GPU too."""
    bh = pkg("bioheat")
    mesh = pkg("boxmesh").BoxMesh(2, (2, 2, 2))
    with pytest.raises(TypeError):
        bh.BioheatSpectral3D(mesh, np.float16)
    for kw in (dict(conductivity=0.0), dict(conductivity=-1.0), dict(density=0.0), dict(specific_heat=float("nan")),
               dict(perfusion_rate=-1e-3), dict(blood_density=-1.0), dict(conductivity=np.ones(mesh.ncells + 1)),
               dict(perfusion_rate=np.ones((mesh.ncells, 2))), dict(fixed_tags=3)):
        with pytest.raises(ValueError):
            bh.BioheatSpectral3D(mesh, np.float64, **kw)


def test_header_and_binding_carry_the_stage_kernel():
    hdr = open(os.path.join(ROOT, "include", "fus_gpu.h")).read()
    sig = pkg("_lib").SIGNATURES
    for suf in ("f64", "f32"):
        assert re.search(rf"\bint fus_bioheat_stage_{suf}\s*\(", hdr)
        assert len(sig[f"fus_bioheat_stage_{suf}"]) == 19
    assert re.search(r"#define FUS_ABI_VERSION 3\b", hdr)
    mk = open(os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc", "Makefile")).read()
    assert "bioheat.hpp" in re.search(r"^HDR = (.*)$", mk, re.M).group(1).split()
    assert "bioheat_stage_kernel" in open(os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc", "bioheat.hpp")).read()


def test_entry_point_validates_before_device_work():
    import ctypes as C

    lib = pkg("_lib").load()
    z, one = C.c_void_p(0), C.c_void_p(256)

    def call(kind=0, minv=one, b=one, T0=one, Tn=one, acc=one, nlocal=4, ntotal=5):
        return lib.fus_bioheat_stage_f64(0.1, 0.1, kind, 1.0, 37.0, 0.1, minv, z, z, b, T0, Tn, acc, z, z, 0, nlocal, ntotal, z)

    assert call(ntotal=0, nlocal=0, minv=z, b=z, T0=z, Tn=z, acc=z) == 0  # no-op
    for kw in (dict(minv=z), dict(b=z), dict(T0=z), dict(Tn=z), dict(acc=z), dict(nlocal=-1), dict(ntotal=-1, nlocal=-2),
               dict(nlocal=6), dict(kind=3), dict(kind=-1), dict(b=C.c_void_p(260))):
        assert call(**kw) == -1, kw
    assert lib.fus_bioheat_stage_f32(0.1, 0.1, 2, 1.0, 37.0, 0.1, one, z, z, one, z, one, one, z, z, 0, 4, 5, z) == -1


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_stage_kernel_resource_usage():
    """every instantiation (2 types x (16-byte, scalar) x 3 streaming policies x (FIRST / MIDDLE, LAST)) holds 8 waves
    per SIMD without scratch or LDS (the remarks of tests/test_resource_usage.py, cached under csrc/_asm)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    rows = {k: v for k, v in ru.parse(ru.cached_remarks()).items() if "bioheat_stage_kernel<" in k}
    assert len(rows) == 24, sorted(rows)
    for name, d in rows.items():
        assert d["occupancy"] >= 8 and d["scratch"] == 0 and d["lds"] == 0 and d["agpr"] == 0 and d["vgpr"] <= 64, (name, d)
