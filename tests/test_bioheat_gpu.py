"""Pennes bioheat on the GPU: the stage kernel (fus_bioheat_stage_*) against numpy, BioheatSpectral3D against the CPU loop of
tests/bioheat_cpu.py and against closed forms, its stability bound, partitioned runs, and the chain from the Westervelt solver's
field monitor to temperature and dose."""

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import bioheat_cpu as bc
from conftest import ROOT, TOL, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

RHO_C = 1050.0 * 3600.0
RHO_B_C_B = 1060.0 * 3617.0
LN4 = math.log(4.0)
EPS64 = np.finfo(np.float64).eps


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---- 1. the stage kernel against numpy -----------------------------------------------------------------------------------------
def _stage_case(kind, dtype, shift, ntotal, nlocal, with_pr, with_s, with_cem, with_tmax, init, seed=0, figures=None):
    """Launch one stage through _lib on random operands (every operand sliced ``shift`` elements into its allocation) and check
    every vector against the fp64 reference: outputs within 8 eps sum|terms|, b zero over [0, ntotal), the rest bitwise.  Returns
    every vector as the launch left it."""
    import torch

    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(seed)
    eps = np.finfo(dtype).eps
    r = lambda lo, hi, n=ntotal: rng.uniform(lo, hi, n).astype(dtype)  # noqa: E731
    host = dict(minv=r(0.5, 2.0), b=r(-3.0, 3.0), T0=r(36.0, 50.0), Tn=r(36.0, 50.0), acc=r(36.0, 50.0), pr=r(0.0, 0.5), s=r(0.0, 4.0),
                tmax=r(36.0, 50.0, nlocal))
    cem_host = rng.uniform(0.0, 30.0, nlocal)
    # scalars as the entry point receives them (ctypes rounds to the field type)
    dt = 0.37  # a double in the ABI for either field type
    bw, aw, gate, Ta = (float(dtype(x)) for x in (dt / 6.0, dt / 2.0, 0.7, 37.0))
    dv = {}
    for k, a in list(host.items()) + [("cem43", cem_host)]:
        buf = torch.zeros(a.size + shift, dtype=torch.float64 if k == "cem43" else lib_mod.torch_dtype(dtype), device="cuda")
        dv[k] = buf[shift:]
        dv[k].copy_(_dev(a))
        assert dv[k].data_ptr() % 16 == (shift * dv[k].element_size()) % 16
    ptr = lambda k, on=True: dv[k].data_ptr() if on else None  # noqa: E731
    fn = getattr(lib, f"fus_bioheat_stage_{'f64' if dtype == np.float64 else 'f32'}")
    rc = fn(bw, aw, kind, gate, Ta, dt, ptr("minv"), ptr("pr", with_pr), ptr("s", with_s), ptr("b"), ptr("T0"), ptr("Tn"), ptr("acc"),
            ptr("cem43", with_cem), ptr("tmax", with_tmax), int(init), nlocal, ntotal, lib_mod.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in dv.items()}
    n = nlocal
    own = {k: host[k][:n] for k in ("minv", "b", "T0", "Tn", "acc", "pr", "s")}
    ref, terms = bc.stage_reference(kind, bw, aw, gate, Ta, dt, own["minv"], own["b"], own["T0"], own["Tn"], own["acc"],
                                    pr=own["pr"] if with_pr else None, s=own["s"] if with_s else None,
                                    cem43=cem_host if (with_cem and kind == 2) else None, init=init)
    assert np.all(got["b"] == 0.0), "b must be zero over [0, ntotal)"
    written = {"b"}
    for name in ("T0", "Tn", "acc"):
        if name in ref:
            written.add(name)
            err = np.abs(got[name][:n].astype(np.float64) - ref[name])
            assert np.all(err <= 8 * eps * terms[name]), (name, float(np.max(err / terms[name])) / eps)
            assert np.array_equal(got[name][n:], host[name][n:]), f"{name}: ghost entries touched"
    if kind == 2:
        Tnew = got["T0"][:n]
        if with_tmax:
            written.add("tmax")
            assert np.array_equal(got["tmax"], Tnew if init else np.maximum(host["tmax"], Tnew))
        if with_cem:
            written.add("cem43")
            # against the reference's dose: relative ln 4 |dT| + 4 eps of the field type (the first-order sensitivity of R^(43 - T) to
            # the admitted temperature difference; its second-order term, (ln 4 dT)^2 / 2 ~ 1e-12 for an fp32 field, is above 4 eps of
            # double but far below 4 eps of the field) ...
            dT = np.abs(Tnew.astype(np.float64) - ref["T0"])
            assert np.all(np.abs(got["cem43"] - ref["cem43"]) <= (LN4 * dT + 4 * eps) * ref["cem43"])
            # ... and against the rule applied in fp64 to the kernel's OWN new T0: 4 eps of double (exp2 of either side within one
            # ulp, one product and one sum on either side)
            own_dose = bc.dose_increment(Tnew, dt) + (0.0 if init else cem_host)
            assert np.all(np.abs(got["cem43"] - own_dose) <= 4 * EPS64 * own_dose)
    for name in set(got) - written:  # untouched outputs and every input: bitwise unchanged
        assert np.array_equal(got[name], cem_host if name == "cem43" else host[name]), f"{name} changed"
    if figures is not None:  # the largest error as a ratio to its bound, per output (tests/test_stream_builds_gpu.py prints them)
        for name in ("T0", "Tn", "acc"):
            if name in ref:
                figures[name] = float(np.max(np.abs(got[name][:n].astype(np.float64) - ref[name]) / (8 * eps * terms[name])))
        if kind == 2 and with_cem:
            figures["cem43"] = float(np.max(np.abs(got["cem43"] - own_dose) / (4 * EPS64 * own_dose)))
    return got


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one-element-in"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["FIRST", "MIDDLE", "LAST"])
def test_stage_kernel_against_numpy(kind, dtype, shift):
    """ntotal = 1003, nlocal = 997: odd (the scalar tail) with a ghost block of b; sliced one element in, no operand is 16-byte
    aligned and the W = 1 kernel runs.  With and without each of pr, s, cem43, tmax; init on and off."""
    dose = [(c, t, i) for c in (False, True) for t in (False, True) for i in (False, True)] if kind == 2 else [(False, False, False)]
    for with_pr in (False, True):
        for with_s in (False, True):
            for with_cem, with_tmax, init in dose:
                _stage_case(kind, dtype, shift, 1003, 997, with_pr, with_s, with_cem, with_tmax, init, seed=kind + 3 * shift)


def test_stage_kernel_streaming_size():
    """3 276 800 fp64 dofs (26.2 MB per operand, above stream_shape.hpp's 24 MB threshold): the non-temporal instantiation."""
    _stage_case(2, np.float64, 0, 3_276_800, 3_276_800 - 1001, True, True, True, True, False, seed=9)


# ---- 2. the solver against the CPU loop ------------------------------------------------------------------------------------------
def _two_thermal_materials(mesh):
    """Two materials, a slab across the middle third in x (as test_solver_gpu._two_materials): soft tissue around bone-like tissue."""
    L = mesh.length[0]
    xc = mesh.x_g[mesh.x_dofs].mean(axis=1)[:, 0]
    slab = (xc > L / 3) & (xc < 2 * L / 3)
    assert 0 < slab.sum() < mesh.ncells
    return dict(k=np.where(slab, 0.32, 0.5), rho=np.where(slab, 1900.0, 1050.0), C=np.where(slab, 1300.0, 3600.0), slab=slab)


@functools.lru_cache(maxsize=None)
def _reference_run(P, cells, perturb, length=1.0, steps=12):
    """The CPU loop on the serial mesh, computed once per mesh: heterogeneous k, rho C and w_b, a smooth random q, power on until
    the middle of the run.  Perfusion and q are scaled from the mesh's own lambda_max so that every term matters: pr = 0.05 / 0.2
    lambda_max, and q is sized to heat by 32 K over the on-time without losses (perfusion at these rates leaves a few K of that)."""
    mesh = pkg("boxmesh").BoxMesh(P, cells, perturb=perturb, length=length)
    m = _two_thermal_materials(mesh)
    rho_c = m["rho"] * m["C"]
    lam = bc.CpuBioheat(mesh, m["k"], rho_c).lambda_max()
    wb = np.where(m["slab"], 0.05, 0.2) * lam * rho_c / RHO_B_C_B  # perfusion rate per cell
    dt_guess = 0.8 * 2.785 / (1.25 * lam)
    q = 32.0 * rho_c.min() / (0.5 * steps * dt_guess) * bc.smooth_field(mesh, 11)
    # the solvers take the vertex coordinates in their field type, as LinearSpectral3D does: the same box with fp32 coordinates
    mesh32 = pkg("boxmesh").BoxMesh(P, cells, perturb=perturb, length=length, dtype=np.float32)
    return dict(mesh=mesh, mesh32=mesh32, m=m, wb=wb, q=q, cpu_args=(m["k"], rho_c, wb * RHO_B_C_B), runs={})


def _cpu_result(ref, dt, steps):
    key = (dt, steps)
    if key not in ref["runs"]:
        cpu = bc.CpuBioheat(ref["mesh"], *ref["cpu_args"])
        cpu.set_heat_source(ref["q"])
        cpu.advance(0.0, steps * dt, dt, power=(0.0, 0.5 * steps * dt), max_steps=steps)
        ref["runs"][key] = (cpu.T.copy(), cpu.cem43.copy())
    return ref["runs"][key]


def _check_against_cpu(T, cem, T_ref, cem_ref, dtype, Ta=37.0):
    tol = TOL[np.dtype(dtype)]
    assert np.max(np.abs(T_ref - Ta)) > 1.0  # the run heated
    print(f"T - Ta: rel l2 {rel_l2(T - Ta, T_ref - Ta):.3e} rel max {rel_max(T - Ta, T_ref - Ta):.3e}; "
          f"cem43 rel {np.max(np.abs(cem / cem_ref - 1.0)):.3e}")
    assert rel_l2(T - Ta, T_ref - Ta) < tol["l2"] and rel_max(T - Ta, T_ref - Ta) < tol["mx"]
    assert np.max(np.abs(cem / cem_ref - 1.0)) <= 2 * LN4 * tol["mx"] * np.max(np.abs(T_ref))


SOLVER_CASES = [(2, (3, 2, 2), 0.15), (3, (3, 2, 2), 0.15), (4, (3, 2, 2), 0.15), (3, (4, 4, 4), 0.15)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("geometry", ["G-array", "in-kernel"])
@pytest.mark.parametrize("P,cells,perturb", SOLVER_CASES, ids=[f"P{c[0]}-{'x'.join(map(str, c[1]))}" for c in SOLVER_CASES])
def test_solver_against_cpu_loop(P, cells, perturb, geometry, dtype):
    import torch

    torch.cuda.set_device(0)
    bh = pkg("bioheat")
    ref = _reference_run(P, cells, perturb)
    mesh, m = ref["mesh" if dtype == np.float64 else "mesh32"], ref["m"]
    th = bh.BioheatSpectral3D(mesh, dtype, conductivity=m["k"], density=m["rho"], specific_heat=m["C"], perfusion_rate=ref["wb"],
                              in_kernel_geometry=(geometry == "in-kernel"))
    assert not th.affine and th.in_kernel_geometry == (geometry == "in-kernel")
    th.set_heat_source(ref["q"])
    dt, steps = th.stable_time_step(), 12
    t, done = th.advance(0.0, steps * dt, dt, power=(0.0, 0.5 * steps * dt), max_steps=steps)
    assert done == steps
    T_ref, cem_ref = _cpu_result(ref, dt, steps)
    _check_against_cpu(th.T_sol().astype(np.float64), th.cem43().cpu().numpy(), T_ref, cem_ref, dtype)
    assert np.array_equal(th.peak_temperature().cpu().numpy() >= th.T_sol(), np.ones(mesh.nlocal, bool))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_solver_against_cpu_loop_affine_form(dtype):
    """The third geometry form the constructor can select: the constant-G fast path, on the unperturbed box."""
    import torch

    torch.cuda.set_device(0)
    ref = _reference_run(3, (3, 2, 2), 0.0)
    mesh, m = ref["mesh" if dtype == np.float64 else "mesh32"], ref["m"]
    th = pkg("bioheat").BioheatSpectral3D(mesh, dtype, conductivity=m["k"], density=m["rho"], specific_heat=m["C"], perfusion_rate=ref["wb"])
    assert th.affine and not th.in_kernel_geometry
    th.set_heat_source(_dev(ref["q"]))
    dt, steps = th.stable_time_step(), 12
    th.advance(0.0, steps * dt, dt, power=(0.0, 0.5 * steps * dt), max_steps=steps)
    T_ref, cem_ref = _cpu_result(ref, dt, steps)
    _check_against_cpu(th.T_sol().astype(np.float64), th.cem43().cpu().numpy(), T_ref, cem_ref, dtype)


# ---- 3. closed forms ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    mesh = pkg("boxmesh").BoxMesh(3, (3, 2, 2), perturb=0.15)
    return mesh, bc.CpuBioheat(mesh, 0.5, RHO_C).lambda_max()


def test_heat_is_conserved_and_the_source_adds_exactly(small):
    """(a) w_b = 0, q = 0, random initial field: sum_d m_d T_d is conserved to 1e-13 relative over 20 steps (K 1 = 0, K symmetric);
    with a constant gate it grows by dt sum_d vol_d q_d per step."""
    import torch

    torch.cuda.set_device(0)
    mesh, _ = small
    th = pkg("bioheat").BioheatSpectral3D(mesh, np.float64, initial_temperature=37.0 + 8.0 * np.random.default_rng(1).random(mesh.nlocal))
    mc, vol = th.mc.cpu().numpy().astype(np.float64), th.vol[: mesh.nlocal].cpu().numpy().astype(np.float64)
    dt = th.stable_time_step()
    heat0 = math.fsum(mc * th.T_sol())
    th.advance(0.0, 20 * dt, dt, max_steps=20)
    print("conservation:", (math.fsum(mc * th.T_sol()) - heat0) / heat0)
    assert abs(math.fsum(mc * th.T_sol()) - heat0) <= 1e-13 * heat0
    q = 2.0 * RHO_C / dt * bc.smooth_field(mesh, 3)
    th.set_heat_source(q)
    for _ in range(3):
        before = math.fsum(mc * th.T_sol())
        th.advance(0.0, dt, dt)
        grown = math.fsum(mc * th.T_sol()) - before
        print("growth:", (grown - dt * math.fsum(vol * q)) / before)
        assert abs(grown - dt * math.fsum(vol * q)) <= 1e-13 * before


def test_uniform_perfusion_decays_by_the_rk4_polynomial(small):
    """(b) uniform T_a + 5, uniform perfusion, q = 0: every dof is T_a + 5 rho(z)^n, z = pr dt.  Tolerance: the uniform field
    is in the kernel of K up to rounding, 64 n eps max|T| bounds what n steps of dt lambda_max <= 2.8 make of it."""
    import torch

    torch.cuda.set_device(0)
    mesh, lam = small
    wb = 0.05 * lam * RHO_C / RHO_B_C_B
    th = pkg("bioheat").BioheatSpectral3D(mesh, np.float64, perfusion_rate=wb, initial_temperature=42.0)
    dt, n = th.stable_time_step(), 10
    th.advance(0.0, n * dt, dt, max_steps=n)
    pr = float(th.pr[0].item())
    assert abs(pr / (0.05 * lam) - 1.0) < 1e-12
    expect = 37.0 + 5.0 * bc.rk4_growth(pr * dt) ** n
    assert 37.5 < expect < 41.5
    assert np.max(np.abs(th.T_sol() - expect)) <= 64 * n * EPS64 * 42.0


@pytest.mark.parametrize("T,factor", [(45.0, 4.0), (41.0, 1.0 / 16.0), (43.0, 1.0)])
def test_uniform_field_stays_uniform_and_its_dose_is_closed_form(small, T, factor):
    """(c) no perfusion, no source: the field stays uniform, cem43 after n steps is n dt / 60 R^(43 - T), tmax is the field."""
    import torch

    torch.cuda.set_device(0)
    mesh, _ = small
    th = pkg("bioheat").BioheatSpectral3D(mesh, np.float64, initial_temperature=T)
    dt, n = th.stable_time_step(), 9
    assert float(th.cem43().max().item()) == 0.0
    th.advance(0.0, n * dt, dt, max_steps=n)
    tol = 64 * n * EPS64 * T
    assert np.max(np.abs(th.T_sol() - T)) <= tol
    assert np.max(np.abs(th.peak_temperature().cpu().numpy() - T)) <= tol
    assert np.max(np.abs(th.cem43().cpu().numpy() / (n * dt / 60.0 * factor) - 1.0)) <= LN4 * tol + 4 * EPS64
    th.reset_dose()
    th.advance(0.0, dt, dt)
    assert np.max(np.abs(th.cem43().cpu().numpy() / (dt / 60.0 * factor) - 1.0)) <= LN4 * tol + 4 * EPS64


def test_fixed_tags_hold_their_dofs(small):
    """(d) the dofs of the tagged facets are bitwise unchanged after 10 heated steps, interior dofs moved."""
    import torch

    torch.cuda.set_device(0)
    mesh, _ = small
    T0 = 37.0 + 0.01 * np.random.default_rng(4).random(mesh.nlocal)
    th = pkg("bioheat").BioheatSpectral3D(mesh, np.float64, initial_temperature=T0, fixed_tags=(2, 3))
    fixed = np.unique(mesh.facet_dofmap(mesh.boundary_facets([2, 3])))
    dt = th.stable_time_step()
    th.set_heat_source(np.full(mesh.nlocal, 1.0 * RHO_C / dt))  # 1 K per step
    th.advance(0.0, 10 * dt, dt, max_steps=10)
    T = th.T_sol()
    assert fixed.size > 0 and np.array_equal(T[fixed], T0[fixed])
    free = np.setdiff1d(np.arange(mesh.nlocal), fixed)
    assert np.min(T[free] - T0[free]) > 0.1


# ---- 4. the stability bound --------------------------------------------------------------------------------------------------------
def test_stable_time_step_against_dense_eigenvalues():
    import torch

    torch.cuda.set_device(0)
    mesh = pkg("boxmesh").BoxMesh(2, (3, 2, 2), perturb=0.15)
    cpu = bc.CpuBioheat(mesh, 0.5, RHO_C)
    lam = float(np.linalg.eigvals(cpu.dense_minv_K()).real.max())
    rng = np.random.default_rng(1)
    th = pkg("bioheat").BioheatSpectral3D(mesh, np.float64, initial_temperature=37.0 + 8.0 * rng.random(mesh.nlocal))
    dt1 = th.stable_time_step(safety=1)
    print("stable_time_step(1) * lambda_max / 2.785 =", dt1 * lam / 2.785)
    assert abs(dt1 * lam / 2.785 - 1.0) < 0.05
    lo, hi = float(th.T_sol().min()), float(th.T_sol().max())
    dt = th.stable_time_step(safety=0.8)
    assert abs(dt / dt1 - 0.8) < 1e-12  # float atomics reorder the sums of two runs
    for _ in range(5):
        th.advance(0.0, 10 * dt, dt, max_steps=10)
        T = th.T_sol()
        assert lo <= T.min() and T.max() <= hi
    assert T.max() - T.min() < 0.5 * (hi - lo)  # and it diffused


def test_advance_warns_once_above_the_limit():
    import torch

    torch.cuda.set_device(0)
    mesh = pkg("boxmesh").BoxMesh(2, (2, 2, 2))
    th = pkg("bioheat").BioheatSpectral3D(mesh, np.float64)
    dt1 = th.stable_time_step(safety=1)
    with pytest.warns(RuntimeWarning, match="stability limit"):
        th.advance(0.0, 1.5 * dt1, 1.5 * dt1)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        th.advance(0.0, 1.5 * dt1, 1.5 * dt1)  # once
    with pytest.raises(pkg("_lib").FusGpuError):
        th.set_heat_source(torch.zeros(mesh.nlocal, dtype=torch.float64))  # a host tensor: no CPU fallback


# ---- 5. partitioned ----------------------------------------------------------------------------------------------------------------
_lockstep = pkg("solver_base").run_lockstep


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 1)], ids=["2ranks", "4ranks"])
def test_partitioned_against_serial_cpu_loop(grid):
    import torch

    torch.cuda.set_device(0)
    boxmesh, bh, scat, utils = pkg("boxmesh"), pkg("bioheat"), pkg("scatterer"), pkg("utils")
    P, cells = 3, (4, 4, 4)
    R = int(np.prod(grid))
    ref = _reference_run(P, cells, 0.0)
    serial, m = ref["mesh"], ref["m"]
    meshes = [boxmesh.BoxMesh(P, cells, grid=grid, rank=r) for r in range(R)]
    od, gd = utils.compute_scatterer_data_all([mm.index_map for mm in meshes])
    slab_of = lambda mm: _two_thermal_materials(mm)["slab"]  # noqa: E731
    lam = bc.CpuBioheat(serial, *ref["cpu_args"][:2]).lambda_max()
    solvers = []
    for r, mm in enumerate(meshes):
        mr = _two_thermal_materials(mm)
        wb = np.where(slab_of(mm), 0.05, 0.2) * lam * (mr["rho"] * mr["C"]) / RHO_B_C_B
        solvers.append(bh.BioheatSpectral3D(mm, np.float64, conductivity=mr["k"], density=mr["rho"], specific_heat=mr["C"], perfusion_rate=wb,
                                            comm=scat.NativeComm(local=(7300 + R, R, r)), halo_plan=(od[r], gd[r]), defer_setup_exchange=True))
    with pytest.raises(pkg("_lib").FusGpuError, match="complete the set-up exchange first"):
        solvers[0].set_heat_source(np.zeros(meshes[0].nlocal))
    _lockstep([s._setup for s in solvers])
    for s in solvers:  # minv = fl(1 / mc) on the free dofs: fl(minv mc) = (1 + d1)(1 + d2), |d| <= eps / 2
        free = s._free == 1
        assert bool(free.any()) and float((s.minv[: s.nlocal] * s.mc - 1.0)[free].abs().max().item()) <= 2 * EPS64
    lex = [mm.global_lexicographic_ids()[: mm.nlocal] for mm in meshes]
    lex_serial = serial.global_lexicographic_ids()
    at = np.empty(serial.ndofs, dtype=np.int64)
    at[lex_serial] = np.arange(serial.ndofs)  # global lexicographic id -> serial dof
    for s, ids in zip(solvers, lex):
        s.set_heat_source(ref["q"][at[ids]])
    shared = bh.InProcessGather(R)
    dts = _lockstep([s.stable_time_step_schedule(0.8, reduce=shared) for s in solvers])
    assert max(dts) == min(dts)
    serial_solver = bh.BioheatSpectral3D(serial, np.float64, conductivity=m["k"], density=m["rho"], specific_heat=m["C"], perfusion_rate=ref["wb"])
    dt_serial = serial_solver.stable_time_step(0.8)
    vol, vol_serial = (math.fsum(np.concatenate([s.vol[: s.nlocal].cpu().numpy() for s in ss])) for ss in (solvers, [serial_solver]))
    assert abs(vol / vol_serial - 1.0) <= 1e-13
    print("stable_time_step: ranks", dts[0], "serial", dt_serial)
    assert abs(dts[0] / dt_serial - 1.0) < 0.01
    dt, steps = dts[0], 12
    res = _lockstep([s.advance_schedule(0.0, steps * dt, dt, power=(0.0, 0.5 * steps * dt), max_steps=steps) for s in solvers])
    torch.cuda.synchronize()
    for s in solvers:
        s.check_halo_health()
    assert all(r_[1] == steps for r_ in res)
    T_ref, cem_ref = _cpu_result(ref, dt, steps)
    seen = np.zeros(serial.ndofs, dtype=int)
    for s, ids in zip(solvers, lex):
        seen[at[ids]] += 1
        _check_against_cpu(s.T_sol(), s.cem43().cpu().numpy(), T_ref[at[ids]], cem_ref[at[ids]], np.float64)
    assert np.all(seen == 1)


# ---- 6. the chain: pressure -> heat -> temperature -> dose ----------------------------------------------------------------------------
def test_chain_from_westervelt_monitor_to_temperature():
    """One period of the Westervelt solver -> heat_source_from -> BioheatSpectral3D on the same mesh (w_b = 0): the heat in the
    tissue, sum_d m_d (T_d - T_a), is t_on sum_d vol_d q_d.

    The balance is checked to the 1e-11 the model admits on a run whose T_a and initial temperature are 0: there T IS the rise.
    One windowed period of this source deposits q <= 110 W/m^3, a rise of 2e-5 K per step; stored as a temperature near 37 the
    rise is resolved to eps 37 = 4e-15 K per rounding, 2e-10 of a step's rise, and the sum over the dofs measures the number
    format (7e-10 measured), not the integrator.  The run at 37 is kept, with the bound that format gives.  Per step a dof's T
    takes the roundings of its own storage (4 stages, at most eps |T| together) and of the operator, dt minv (K T)_d, whose terms
    sum to at most 2 dt lambda_max |T| in magnitude (sum_j |K_dj| <= 2 K_dd, minv_d K_dd <= lambda_max, dt lambda_max = 0.8 x
    2.785): at most eps |T| (2 + 2 dt lambda_max).  Taken as the standard deviation of independent errors over dofs and steps,
    m-weighted, and admitted up to 8 of them."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, nl, ls, fm, bh = pkg("boxmesh"), pkg("nonlinear_solver"), pkg("linear_solver"), pkg("field_monitor"), pkg("bioheat")
    P, L, c0, f0 = 3, 0.012, 1480.0, 1.1e6  # the Westervelt solver's default medium and frequency
    mesh = boxmesh.BoxMesh(P, (4, 4, 4), length=L)
    wave = nl.WesterveltSpectral3D(mesh, np.float64, fused=True)
    h = ls.time_step_parameters(mesh, P, c0, f0, L)
    dt_w, _, _ = ls.snap_time_step(h, P, c0, f0, L)
    spp = int(round(1.0 / f0 / dt_w))
    mon = fm.FieldMonitor(wave.nlocal, np.float64, mean_square="v")
    wave.init()
    wave.rk4(0.0, spp * dt_w, dt_w, max_steps=spp, monitor=mon)
    th = bh.BioheatSpectral3D(mesh, np.float64)
    rise = bh.BioheatSpectral3D(mesh, np.float64, arterial_temperature=0.0, initial_temperature=0.0)
    q = bh.heat_source_from(mon, wave, th)
    assert q.is_cuda and q.dtype == torch.float64 and tuple(q.shape) == (th.nlocal,) and float(q.max().item()) > 0.0
    other = bh.BioheatSpectral3D(boxmesh.BoxMesh(P, (3, 4, 4), length=L), np.float64)
    with pytest.raises(ValueError):
        bh.heat_source_from(mon, wave, other)
    th.set_heat_source(q)
    dt = th.stable_time_step()
    rise.set_heat_source(q)
    t_on = 40.5 * dt  # the last step is shortened
    mc, vol = th.mc.cpu().numpy(), th.vol[: th.nlocal].cpu().numpy()
    deposited = t_on * math.fsum(vol * q.cpu().numpy())
    for solver, Ta in ((rise, 0.0), (th, 37.0)):
        t, steps = solver.advance(0.0, t_on, dt)
        assert steps == 41 and abs(t - t_on) <= 1e-14 * t_on
        heat = math.fsum(mc * (solver.T_sol() - Ta))
        print(f"chain, T_a = {Ta}: heat / deposited - 1 = {heat / deposited - 1.0:.3e}")
        if Ta == 0.0:
            assert abs(heat / deposited - 1.0) <= 1e-11
        else:
            sigma = EPS64 * (2.0 + 2.0 * 0.8 * 2.785) * math.sqrt(steps) * float(np.linalg.norm(mc * solver.T_sol()))
            print(f"chain, T_a = 37: |heat - deposited| = {abs(heat - deposited):.3e}, 8 sigma = {8 * sigma:.3e}")
            assert abs(heat - deposited) <= 8 * sigma
    foc = fm.focus(th.cem43(), th, level=0.5)
    assert foc["max"] > 0.0 and foc["volume"] > 0.0


DEMO_ARGS = ("--degree", "3", "--cells", "4", "--length", "0.004", "--thermal", "2", "1")  # the smallest mesh the demo's tests run


def test_demo_thermal_flag_prints_finite_numbers():
    """demo_nonlinear_bowl.py --thermal at its smallest mesh: peak temperature, dose focus and lesion volume are printed and finite."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fenicsx-fus-gpu_amd", "demo_nonlinear_bowl.py"), *DEMO_ARGS],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    vals = {}
    for line in r.stdout.splitlines():
        if line.startswith("thermal:"):
            for item in line[len("thermal:"):].split(","):
                k, v = item.split("=")
                vals[k.strip()] = float(v.split()[0])
    assert {"peak temperature", "max cem43", "volume above 240 cem43"} <= set(vals), r.stdout[-3000:]
    assert all(np.isfinite(v) for v in vals.values()) and vals["peak temperature"] >= 37.0

