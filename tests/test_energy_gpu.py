"""Energy records, the field guard and the operator-based stable step of the two wave solvers on the GPU, against the CPU wave model
and its dense operators (tests/wave_energy_cpu.py) on the smallest meshes that have interior, shared and boundary dofs: P = 2 on
(3, 2, 2) perturbed cells, P = 4 (P = 3 for Westervelt) on (2, 2, 2)."""
import functools
import warnings

import numpy as np
import pytest

import test_energy as cpu_cases
import wave_energy_cpu as we
from conftest import TOL, pkg

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

_lockstep = pkg("solver_base").run_lockstep


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to("cuda")


def _set_state(solver, u, v):
    solver.init()
    solver.u.copy_(_dev(u, solver.tdt_np))
    solver.v.copy_(_dev(v, solver.tdt_np))


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- the solvers of the energy-value check, each with the dense operators of its medium ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(kind):
    """``(solver, dense model)``; the model is built once per kind and left unchanged."""
    ls, nl, nm = pkg("linear_solver"), pkg("nonlinear_solver"), pkg("nodal_medium")
    torch.cuda.set_device(0)
    quiet = dict(source_frequency=we.F0, source_amplitude=0.0)
    if kind in ("linear-f64", "linear-f32", "linear-reference-sequence"):
        ft = np.float32 if kind == "linear-f32" else np.float64
        mesh = we.box(dtype=ft)
        c, rho = we.two_materials(mesh)
        dense = we.Dense(we.box(), "linear", c, rho)
        return ls.LinearSpectral3D(mesh, ft, speed_of_sound=c, density=rho, fused=kind != "linear-reference-sequence", **quiet), dense
    if kind in ("linear-P4", "linear-G-array"):
        mesh = we.box(P=4, cells=(2, 2, 2), perturb=0.1, seed=5)
        c, rho = we.two_materials(mesh)
        s = ls.LinearSpectral3D(mesh, np.float64, speed_of_sound=c, density=rho, in_kernel_geometry=kind == "linear-P4", **quiet)
        assert s.in_kernel_geometry == (kind == "linear-P4")
        return s, we.Dense(mesh, "linear", c, rho)
    if kind == "linear-nodal":
        mesh = we.box()
        x = np.asarray(mesh.dof_coordinates(), dtype=np.float64)[:, 0] / we.LENGTH
        c_n, rho_n = 1500.0 + 1300.0 * x * x, 1000.0 + 850.0 * x  # water at the source face, bone at the far one
        s = ls.LinearSpectral3D(mesh, np.float64, nodal_medium=nm.NodalMedium(c_n, rho_n), **quiet)
        return s, we.Dense(mesh, "linear", nm.cell_means(c_n, mesh.dofmap), nm.cell_means(rho_n, mesh.dofmap), nodal=(c_n, rho_n))
    if kind == "westervelt-P3":
        mesh = we.box(P=3, cells=(2, 2, 2), perturb=0.1, seed=5)
        c, rho = we.two_materials(mesh)
        s = nl.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=c, density=rho, attenuation_coefficient_dB=50.0, fused=True, **quiet)
        return s, we.Dense(mesh, "westervelt", c, rho, att_dB=50.0)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["linear-f64", "linear-f32", "linear-P4", "linear-G-array", "linear-nodal", "westervelt-P3",
                                  "linear-reference-sequence"])
def test_energy_record_equals_the_energy_of_the_field(kind):
    """After k = 1, 2, 3 steps from a seeded smooth state the last record equals 1/2 v.M v + 1/2 u.K u formed in numpy from u_sol(),
    v_sol() and the oracle's dense K and lumped mass, to the project's parity bar (relative)."""
    solver, dense = _case(kind)
    rec = pkg("diagnostics").EnergyRecorder(solver, capacity=8)
    u0, v0 = we.smooth_state(dense.mesh, seed=4)
    dt, tol = 0.5 * dense.formula(1.0), TOL[np.dtype(solver.tdt_np)]["mx"]
    for k in (1, 2, 3):
        _set_state(solver, u0, v0)
        rec.reset()
        t_end, steps = solver.rk4(0.0, 1.0, dt, max_steps=k, energy=rec)
        assert steps == k and rec.nrec == k
        t, kin, pot, tot, amax, bad = rec.energies()
        u, v = solver.u_sol(), solver.v_sol()
        kin_ref, pot_ref = dense.energy(u, v)
        print(f"{kind} k={k}: kinetic {kin[-1]:.12e} ({_rel(kin[-1], kin_ref):.2e}), potential {pot[-1]:.12e} ({_rel(pot[-1], pot_ref):.2e})")
        assert _rel(kin[-1], kin_ref) <= tol and _rel(pot[-1], pot_ref) <= tol and _rel(tot[-1], kin_ref + pot_ref) <= tol
        assert t[-1] == t_end and amax[-1] == float(np.abs(u).max()) and bad[-1] == 0.0
        assert np.all(np.diff(t) > 0) and pot[-1] > 0.0 and kin[-1] > 0.0


def test_series_bookkeeping():
    """Times are the recorded steps' ``record_times``; ``every`` thins them; a full series stops and the run goes on; ``record_from``
    is respected; the recorder's scratch is its own (the field and the solver's b are as a run without it leaves them, to the parity
    bar: the apply's float atomics reorder from run to run)."""
    solver, dense = _case("linear-f64")
    diag, recording = pkg("diagnostics"), pkg("recording")
    u0, v0 = we.smooth_state(dense.mesh, seed=4)
    dt = 0.5 * dense.formula(1.0)
    times = recording.record_times(0.0, 1.0, dt, 9)
    rec = diag.EnergyRecorder(solver, every=2, capacity=3)
    _set_state(solver, u0, v0)
    assert solver.rk4(0.0, 1.0, dt, max_steps=9, energy=rec)[1] == 9
    assert rec.full and rec.nrec == 3 and rec.energies()[0].tolist() == [times[1], times[3], times[5]]  # steps 2, 4, 6; 8 found it full
    u_with, b_with = solver.u_sol().copy(), solver.b.clone()
    _set_state(solver, u0, v0)
    solver.rk4(0.0, 1.0, dt, max_steps=9)
    tol = TOL[np.dtype(np.float64)]["mx"]
    assert np.max(np.abs(u_with - solver.u_sol())) <= tol * np.max(np.abs(u_with))
    assert float((b_with - solver.b).abs().max()) <= tol * float(b_with.abs().max())
    every = diag.EnergyRecorder(solver, capacity=16)
    _set_state(solver, u0, v0)
    solver.rk4(0.0, 1.0, dt, max_steps=9, energy=every, record_from=times[3])
    assert every.energies()[0].tolist() == recording.record_times(0.0, 1.0, dt, 9, record_from=times[3]) == times[4:]
    with pytest.raises(ValueError):
        diag.EnergyRecorder(solver, every=0)


def test_graph_replay_records_the_same_series():
    """rk4_graph: the recorder's launches follow each replay outside the capture.  Same series as rk4 to the parity bar (not bitwise:
    the float atomics of the apply reorder)."""
    solver, dense = _case("linear-f64")
    diag = pkg("diagnostics")
    u0, v0 = we.smooth_state(dense.mesh, seed=4)
    dt, tol = 0.5 * dense.formula(1.0), TOL[np.dtype(np.float64)]["mx"]
    series = []
    for loop in (solver.rk4, solver.rk4_graph):
        rec = diag.EnergyRecorder(solver, capacity=8)
        _set_state(solver, u0, v0)
        assert loop(0.0, 1.0, dt, max_steps=6, energy=rec, guard=diag.FieldGuard(every=3))[1] == 6
        series.append(rec.energies())
    assert series[0][0].tolist() == series[1][0].tolist() and len(series[0][0]) == 6
    for a, b in zip(series[0][1:4], series[1][1:4]):
        assert np.all(np.abs(a - b) <= tol * np.abs(a))


def test_energy_decays_with_the_source_off():
    """The CPU model's energies of this run are non-increasing (tests/test_energy.py checks that first); the device series is then
    non-increasing up to 1e-12 relative per step, ends below where it began, and follows the model."""
    dense, u0, v0, nsteps, dt = cpu_cases.decay_case()
    solver, same = _case("linear-P4")
    assert same.mesh.ndofs == dense.mesh.ndofs
    rec = pkg("diagnostics").EnergyRecorder(solver, capacity=nsteps)
    _set_state(solver, u0, v0)
    solver.rk4(0.0, 1.0, dt, max_steps=nsteps, energy=rec)
    E = rec.energies()[3]
    E0 = sum(dense.energy(u0, v0))
    E_cpu = np.array([sum(dense.energy(*s)) for s in dense.run(u0, v0, nsteps, dt)])
    print("decay: E_last / E_0", E[-1] / E0, "CPU", E_cpu[-1] / E0, "largest step ratio", float(np.max(E[1:] / E[:-1])))
    assert len(E) == nsteps and E[0] <= E0 * (1 + 1e-12) and np.all(E[1:] <= E[:-1] * (1 + 1e-12)) and E[-1] < E0
    assert np.all(np.abs(E - E_cpu) <= TOL[np.dtype(np.float64)]["mx"] * E_cpu)


# ---- the stable step -------------------------------------------------------------------------------------------------------------------
def _configured_solver(name, mesh=None, **kw):
    ls, nl, sp = pkg("linear_solver"), pkg("nonlinear_solver"), pkg("sponge")
    cfg = we.configuration(name)
    mesh = cfg.mesh if mesh is None else mesh
    c, rho = we.two_materials(mesh)
    quiet = dict(source_frequency=we.F0, source_amplitude=0.0)
    if name == "westervelt":
        return nl.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=c, density=rho, attenuation_coefficient_dB=float(cfg.att_dB[0]),
                                       fused=True, **quiet, **kw)
    sponge = sp.SpongeLayer(cfg.sigma_fn) if name == "sponge" else None
    return ls.LinearSpectral3D(mesh, np.float64, speed_of_sound=c, density=rho, sponge=sponge, **quiet, **kw)


@pytest.mark.parametrize("name", ["linear", "sponge", "westervelt"])
def test_stable_time_step_against_exact_eigenvalues(name):
    """stable_time_step(1) agrees with the formula at exact eigenvalues within what bioheat's test allows its estimate (5 % of
    lambda_max, hence 2.5 % of an undamped step; the Lanczos value is a lower bound), stable_time_step(0.8) <= dt*, and rk4 with a
    longer dt warns once."""
    torch.cuda.set_device(0)
    cfg, solver = we.configuration(name), _configured_solver(name)
    assert solver.stable_limit is None
    dt1 = solver.stable_time_step(1.0)
    lam, dmax = cfg.lambda_max(), cfg.damping_max()
    print(f"{name}: lambda_max {solver.lambda_max:.6e} (exact {lam:.6e}), damping_max {solver.damping_max:.6e} (exact {dmax:.6e}), "
          f"stable_time_step(1) {dt1:.6e}, formula {cfg.formula(1.0):.6e}, dt* {cfg.true_limit():.6e}")
    assert 0.95 * lam <= solver.lambda_max <= lam * (1 + 1e-9)
    assert 0.95 * dmax <= solver.damping_max <= dmax * (1 + 1e-9)
    assert cfg.formula(1.0) * (1 - 1e-9) <= dt1 <= 1.025 * cfg.formula(1.0) and dt1 == solver.stable_limit
    assert solver.stable_time_step(0.8) <= cfg.true_limit()
    u0, v0 = we.smooth_state(cfg.mesh, seed=4)
    _set_state(solver, 1e-3 * u0, 1e-3 * v0)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        solver.rk4(0.0, 1.0, 0.9 * solver.stable_limit, max_steps=1)
        assert not caught
        solver.rk4(0.0, 1.0, 1.2 * solver.stable_limit, max_steps=1)
        solver.rk4(0.0, 1.0, 1.2 * solver.stable_limit, max_steps=1)
    assert len(caught) == 1 and issubclass(caught[0].category, RuntimeWarning) and "stability limit" in str(caught[0].message)


def test_two_ranks_energy_and_stable_step():
    """Two in-process ranks in lock step with reduce=InProcessGather(2): the summed energy series equals the serial one to the parity
    bar, the ranks' stable steps agree exactly and with the serial value to 1 %."""
    torch.cuda.set_device(0)
    scat, utils, diag, bh = pkg("scatterer"), pkg("utils"), pkg("diagnostics"), pkg("bioheat")
    serial = _configured_solver("linear")
    meshes = [we.box(grid=(2, 1, 1), rank=r) for r in range(2)]
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    ranks = [_configured_solver("linear", mesh=m, comm=scat.NativeComm(local=(7411, 2, r)), halo_plan=(od[r], gd[r]),
                                defer_setup_exchange=True) for r, m in enumerate(meshes)]
    _lockstep([s._setup for s in ranks])
    shared = bh.InProcessGather(2)
    dts = _lockstep([s.stable_time_step_schedule(1.0, reduce=shared) for s in ranks])
    dt_serial = serial.stable_time_step(1.0)
    print("stable_time_step(1): ranks", dts, "serial", dt_serial)
    assert dts[0] == dts[1] and abs(dts[0] / dt_serial - 1.0) <= 0.01
    dt, nsteps, tol = 0.5 * dt_serial, 4, TOL[np.dtype(np.float64)]["mx"]
    rec_serial = diag.EnergyRecorder(serial, capacity=nsteps)
    _set_state(serial, *we.smooth_state(serial.mesh, seed=4))
    serial.rk4(0.0, 1.0, dt, max_steps=nsteps, energy=rec_serial)
    recs = [diag.EnergyRecorder(s, capacity=nsteps) for s in ranks]
    for s in ranks:
        _set_state(s, *we.smooth_state(s.mesh, seed=4))
    _lockstep([s.rk4_schedule(0.0, 1.0, dt, max_steps=nsteps, energy=r) for s, r in zip(ranks, recs)])
    for s in ranks:
        s.check_halo_health("two ranks")
    shared = bh.InProcessGather(2)
    joined = _lockstep([r.energies_schedule(reduce=shared) for r in recs])
    want = rec_serial.energies()
    for got in joined:
        assert got[0].tolist() == want[0].tolist()
        for a, b in zip(got[1:4], want[1:4]):
            assert np.all(np.abs(a - b) <= tol * np.abs(b)), (a, b)
        assert np.all(np.abs(got[4] - want[4]) <= tol * want[4]) and np.all(got[5] == 0.0)
    assert all(np.array_equal(a, b) for a, b in zip(joined[0], joined[1]))


# ---- the guard -------------------------------------------------------------------------------------------------------------------------
def test_guard_names_the_step_of_a_nan():
    solver, dense = _case("linear-f64")
    diag, FusGpuError = pkg("diagnostics"), pkg("_lib").FusGpuError
    u0, v0 = we.smooth_state(dense.mesh, seed=4)
    u0 = u0.copy()
    u0[solver.nlocal // 2] = np.nan
    _set_state(solver, u0, v0)
    guard = diag.FieldGuard(every=4)
    with pytest.raises(FusGpuError, match=r"FieldGuard: step (\d+), t = .* not finite") as caught:
        solver.rk4(0.0, 1.0, 0.5 * dense.formula(1.0), max_steps=12, guard=guard)
    assert guard.steps <= 4 and f"step {guard.steps}," in str(caught.value) and guard.last[1] >= 1


def test_guard_catches_an_unstable_step_and_passes_a_stable_one():
    """1.5 x stable_time_step(1): arithmetic overflow of the field, nothing the device faults on.  The CPU model of the same run
    says after how many steps max |u| passes 1e6 x the initial amplitude; the guard, asked every 4 steps, must raise by the second
    check after that.  The same run at 0.8 x does not raise."""
    torch.cuda.set_device(0)
    diag, FusGpuError = pkg("diagnostics"), pkg("_lib").FusGpuError
    cfg, u0, v0, limit = cpu_cases.blow_up_case()
    solver = _configured_solver("linear")
    bound = solver.stable_time_step(1.0)
    k_cpu = cpu_cases.steps_to_exceed(cfg, u0, v0, 1.5 * bound, limit, 400)
    assert k_cpu is not None
    every = 4
    guard = diag.FieldGuard(every=every, limit=limit)
    _set_state(solver, u0, v0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(FusGpuError, match="exceeds the limit.*the step is too long") as caught:
            solver.rk4(0.0, 1.0, 1.5 * bound, max_steps=k_cpu + 3 * every, guard=guard)
    print("guard:", caught.value, "| CPU model:", k_cpu, "steps")
    assert k_cpu <= guard.steps <= (k_cpu + every - 1) // every * every + every and guard.steps % every == 0
    calm = diag.FieldGuard(every=every, limit=limit)
    _set_state(solver, u0, v0)
    assert solver.rk4(0.0, 1.0, 0.8 * bound, max_steps=k_cpu + 3 * every, guard=calm)[1] == k_cpu + 3 * every
    assert calm.last[0] <= limit and calm.last[1] == 0


def test_absent_keywords_change_no_bit():
    """guard=None, energy=None against a run without the keywords, on the single-rank fp64 path with the G array (the tuning
    defaults): the same field, bit for bit, if that path's float atomics reproduce from run to run -- two runs WITHOUT the keywords
    say whether they do; if not, the comparison is at the parity bar."""
    solver, dense = _case("linear-G-array")
    u0, v0 = we.smooth_state(dense.mesh, seed=4)
    dt = 0.5 * dense.formula(1.0)
    fields = []
    for kw in ({}, {}, dict(energy=None, guard=None)):
        _set_state(solver, u0, v0)
        solver.rk4(0.0, 1.0, dt, max_steps=5, **kw)
        fields.append((solver.u_sol().copy(), solver.v_sol().copy()))
    reproducible = all(np.array_equal(a, b) for a, b in zip(fields[0], fields[1]))
    print("two plain runs bitwise equal:", reproducible)
    for a, b in zip(fields[0], fields[2]):
        if reproducible:
            assert np.array_equal(a, b)
        else:
            assert np.max(np.abs(a - b)) <= TOL[np.dtype(np.float64)]["mx"] * np.max(np.abs(a))
