"""Shock capturing on the GPU: every shipped build of the sensor kernel against the fp64 model of tests/shock_model.py and its derived
bound, and the Westervelt solver with the attachment against the CPU model of the run, on a thin box (N x 1 x 1 cells, P = 4) whose
rigid lateral walls keep a plane wave planar."""
import ctypes as C
import functools

import numpy as np
import pytest

import shock_model as sm
import wave_energy_cpu as we
from conftest import TOL, pkg, rel_l2

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

_BAR = 1e-11  # the bar of the existing Westervelt solver tests against the CPU loop (test_westervelt_nodal_gpu.py, test_sponge_gpu.py, ...)
DEGREES = list(range(1, 11))


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))).to("cuda")


# ---- the kernel against the model ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh_case(P, kind):
    """``(dofmap, ndofs, fields)``: the perturbed (3, 2, 2) box (the mesh of ``cell_model64.box(P, (3, 2, 2))``, with coordinates) or
    37 cells with random dofmap rows -- no multiple of any cells-per-workgroup count: the last workgroup is partial and cells straddle
    waves.  Fields in fp64: random (top share O(1)), smooth (box only) and all-zero."""
    rng = np.random.default_rng(100 * P + len(kind))
    n3 = (P + 1) ** 3
    if kind == "box":
        mesh = we.box(P=P, cells=(3, 2, 2), perturb=0.2, seed=40 + P)
        dofmap, ndofs = mesh.dofmap, mesh.ndofs
        fields = {"smooth": we.smooth_state(mesh, seed=4)[0]}
    else:
        ndofs = 50 + n3
        dofmap, fields = rng.integers(0, ndofs, size=(37, n3), dtype=np.int32), {}
    fields.update(random=rng.standard_normal(ndofs), zero=np.zeros(ndofs))
    nc = dofmap.shape[0]
    per_cell = dict(cc4_base=-rng.uniform(1e-10, 5e-10, nc), scale=rng.uniform(3e-10, 6e-10, nc), eps_max=rng.uniform(0.01, 0.1, nc))
    return np.ascontiguousarray(dofmap), ndofs, fields, per_cell


def _launch(P, dtype, dofmap_d, u_d, base_d, scale_d, epsmax_d, eps_d, sensor_d, cc4_d, s0, kappa, floor, hold):
    lib_mod = pkg("_lib")
    fn = getattr(lib_mod.load(), f"fus_modal_sensor_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")
    Vinv = _dev(pkg("shock_capture").modal_table(P), dtype)
    lib_mod.check(fn(u_d.data_ptr(), dofmap_d.data_ptr(), Vinv.data_ptr(), base_d.data_ptr(), scale_d.data_ptr(), epsmax_d.data_ptr(),
                     eps_d.data_ptr(), sensor_d.data_ptr(), cc4_d.data_ptr(), P, dofmap_d.shape[0], s0, kappa, floor, hold, C.c_void_p(0)),
                  "fus_modal_sensor")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("P", DEGREES)
@pytest.mark.parametrize("kind", ["box", "random-dofmap"])
def test_kernel_against_the_model(P, dtype, kind):
    """Per field: ``s`` and ``eps`` inside the intervals the derived energy bounds allow (``shock_model.intervals``: the two-sided
    bound of top / tot carried through log10 and the ramp), ``cc4`` from the device's own ``eps`` to two roundings of its type, a
    second launch bitwise equal, and with ``hold`` a launch on a zero field that leaves ``hold eps``.  The kernel returns no energy
    by itself: ``tot`` is held against its bound through the quiet test, with one floor just above the largest and one just below the
    smallest ``tot`` the bound allows.  All-zero: every cell quiet, ``cc4 == cc4_base`` bit for bit and ``eps == 0``."""
    torch.cuda.set_device(0)
    dofmap, ndofs, fields, pc = _mesh_case(P, kind)
    nc = dofmap.shape[0]
    s0, kappa, floor, hold = float(pkg("shock_capture").default_s0(P)), 0.5, 0.01, 0.5
    dm_d = _dev(dofmap)
    base, scale = pc["cc4_base"].astype(dtype), pc["scale"].astype(dtype)
    base_d, scale_d, epsmax_d = _dev(base), _dev(scale), _dev(pc["eps_max"])
    ut = sm.unit_roundoff(dtype)

    def run(u, eps0, floor_=floor, hold_=0.0):
        eps_d, sensor_d, cc4_d = _dev(eps0), _dev(np.full(nc, 7.0)), _dev(np.full(nc, 7.0, dtype=dtype))
        _launch(P, dtype, dm_d, _dev(u), base_d, scale_d, epsmax_d, eps_d, sensor_d, cc4_d, s0, kappa, floor_, hold_)
        return eps_d.cpu().numpy(), sensor_d.cpu().numpy(), cc4_d.cpu().numpy()

    for name, field in fields.items():
        u = field.astype(dtype)  # the values the device holds
        zeros = np.zeros(nc)
        eps, s, cc4 = run(u, zeros)
        again = run(u, zeros)
        assert np.array_equal(eps, again[0]) and np.array_equal(s, again[1]) and np.array_equal(cc4, again[2]), name
        assert np.all(np.isfinite(s)) and np.all(np.isfinite(eps))
        if name == "zero":
            assert np.all(eps == 0.0) and np.all(s == sm.QUIET) and np.array_equal(cc4, base)
            continue
        m = sm.sensor(u, dofmap, P, floor, s0, kappa, pc["eps_max"], dtype=dtype)
        lo, hi, e_lo, e_hi, decided = sm.intervals(m["tot"], m["top"], m["btot"], m["btop"], floor, s0, kappa, pc["eps_max"], zeros, 0.0)
        assert decided.all() and np.all(m["tot"] > 8 * floor * floor), "the case must not sit on the quiet threshold"
        held = s != sm.QUIET
        print(f"P={P} {np.dtype(dtype).name} {kind} {name}: s model {m['s'].min():.3f} .. {m['s'].max():.3f}, largest |s - model| "
              f"{np.max(np.abs(s[held] - m['s'][held])) if held.any() else 0.0:.3e}, widest interval {np.max(hi - np.maximum(lo, -50)):.3e}, "
              f"eps > 0 in {int((eps > 0).sum())}/{nc} cells")
        assert np.all((s[held] >= lo[held]) & (s[held] <= hi[held])), name
        assert np.all(np.isneginf(lo[~held])), name  # the sentinel only where the bound allows top <= 0
        assert np.all((eps >= e_lo) & (eps <= e_hi)), name
        want = base.astype(np.float64) - eps * scale.astype(np.float64)
        assert np.all(np.abs(cc4 - want) <= 2 * ut * np.abs(want)) and np.array_equal(cc4[eps == 0.0], base[eps == 0.0]), name
        if name == "random":
            assert (eps > 0).any()
        # tot against its bound, through the quiet test
        above = np.sqrt((m["tot"] + m["btot"]).max() / 8.0) * (1 + 1e-12)
        below = np.sqrt((m["tot"] - m["btot"]).min() / 8.0) * (1 - 1e-12)
        assert np.all(run(u, zeros, floor_=above)[1] == sm.QUIET)
        loud = run(u, zeros, floor_=below)[1]
        assert np.all((loud != sm.QUIET) | np.isneginf(lo))
        # the hold: a zero field after this one leaves hold * eps, and cc4 follows
        eps2, s2, cc42 = run(np.zeros(ndofs, dtype=dtype), eps, hold_=hold)
        assert np.array_equal(eps2, hold * eps) and np.all(s2 == sm.QUIET)
        want2 = base.astype(np.float64) - eps2 * scale.astype(np.float64)
        assert np.all(np.abs(cc42 - want2) <= 2 * ut * np.abs(want2))


# ---- the solver ------------------------------------------------------------------------------------------------------------------------
def _solver(mesh, p0, capture=None, fused=True, **kw):
    nl = pkg("nonlinear_solver")
    s = nl.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=sm.C0, density=sm.RHO0, source_frequency=sm.F0, source_amplitude=p0,
                                nonlinear_coefficient=sm.BETA, attenuation_coefficient_dB=sm.ATT_DB, fused=fused, shock_capture=capture, **kw)
    if not kw.get("defer_setup_exchange"):
        s.init()
    return s


class _Peak:
    """``max |u|`` over the steps of a run, on the device (handed to rk4 as ``guard=``: asked after every step, no host sync)."""

    def __init__(self):
        self.peak = None

    def expect_steps(self, *a):
        pass

    def check(self, solver, u, t):
        m = u[: solver.nlocal].abs().max()
        self.peak = m if self.peak is None else torch.maximum(self.peak, m)


def _run(solver, case, loop="rk4"):
    solver.init()
    peak = _Peak()
    t, steps = getattr(solver, loop)(0.0, 1.0, case["dt"], max_steps=case["steps"], guard=peak)
    assert steps == case["steps"]
    return solver.u_sol().copy(), solver.v_sol().copy(), float(peak.peak.item()) / case["p0"] - 1.0


@functools.lru_cache(maxsize=None)
def _high_cpu():
    """The captured high-drive run in the CPU model, once: ``(u, v, eps, overshoot)``."""
    case = sm.HIGH_DRIVE
    mesh = sm.thin_box(case["ncells"], case["length"])
    run = sm.Run(mesh, case["p0"], sm.ATT_DB, sm.default_capture(mesh, case["p0"]))
    u, v = run.advance(case["steps"], case["dt"])
    return u, v, run.eps.copy(), run.peak / case["p0"] - 1.0


@functools.lru_cache(maxsize=None)
def _high_gpu(fused=True):
    torch.cuda.set_device(0)
    case = sm.HIGH_DRIVE
    cap = pkg("shock_capture").ShockCapture()
    solver = _solver(sm.thin_box(case["ncells"], case["length"]), case["p0"], cap, fused=fused)
    return solver, cap, _run(solver, case)


def test_low_drive_costs_nothing():
    """The shock distance lies far beyond the box and the mesh resolves the wave: the run with the attachment equals the plain run
    bit for bit in u and v, and no cell ever got any diffusivity."""
    torch.cuda.set_device(0)
    case = sm.LOW_DRIVE
    assert sm.shock_distance(case["p0"]) > 1000 * case["length"]
    cap = pkg("shock_capture").ShockCapture()
    mesh = sm.thin_box(case["ncells"], case["length"])
    plain, again, captured = _solver(mesh, case["p0"]), _solver(mesh, case["p0"]), _solver(mesh, case["p0"], cap)
    a, b, c = _run(plain, case), _run(again, case), _run(captured, case)
    print("low drive: two plain runs bitwise equal:", np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "| launches",
          cap.launches, "| largest sensor value", cap.sensor().max(), "against the ramp's foot", cap.s0 - cap.kappa, "| max |u| / p0", a[2] + 1)
    assert cap.launches == case["steps"] and cap.active_cells() == 0 and np.all(cap.artificial_diffusivity() == 0.0)
    assert torch.equal(captured.cc4, captured.cc4_base) and cap.sensor().max() > sm.QUIET  # the wave was seen, and judged smooth
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_high_drive_overshoot_and_parity():
    """The plain run overshoots above, the captured run below the midpoint of the CPU model's two values; eps per cell
    and the final field of the captured run equal the CPU model's to the parity bar."""
    case = sm.HIGH_DRIVE
    u_cpu, v_cpu, eps_cpu, over_cpu = _high_cpu()
    assert abs(over_cpu - case["overshoot_captured"]) <= 1e-9 * case["overshoot_captured"]
    mid = 0.5 * (case["overshoot_plain"] + case["overshoot_captured"])
    solver, cap, (u, v, over) = _high_gpu()
    plain = _run(_solver(solver.mesh, case["p0"]), case)
    du, dv = rel_l2(u, u_cpu), rel_l2(v, v_cpu)
    eps = cap.artificial_diffusivity()
    de = float(np.max(np.abs(eps - eps_cpu)) / eps_cpu.max())
    print(f"high drive: overshoot plain {plain[2]:.6f} (CPU {case['overshoot_plain']:.6f}), captured {over:.6f} (CPU {over_cpu:.6f}), "
          f"midpoint {mid:.6f}; rel l2 to the CPU model u {du:.3e} v {dv:.3e}; eps {de:.3e} of max, active {cap.active_cells()}")
    assert np.all(np.isfinite(plain[0])) and np.all(np.isfinite(u)) and np.all(np.isfinite(v))
    assert plain[2] > mid > over
    assert cap.active_cells() == int((eps_cpu > 0).sum()) > 0
    assert de <= _BAR and du < _BAR and dv < _BAR


def test_graph_replay_equals_rk4():
    solver, cap, (u, v, over) = _high_gpu()
    u_g, v_g, over_g = _run(solver, sm.HIGH_DRIVE, loop="rk4_graph")
    du, dv = rel_l2(u_g, u), rel_l2(v_g, v)
    print(f"rk4_graph against rk4: u {du:.3e} v {dv:.3e}, overshoot {over_g:.6f} against {over:.6f}")
    assert cap.launches == sm.HIGH_DRIVE["steps"] and du < _BAR and dv < _BAR


def test_reference_sequence_matches_the_model():
    u_cpu, v_cpu, eps_cpu, _ = _high_cpu()
    solver, cap, (u, v, over) = _high_gpu(fused=False)
    du, dv = rel_l2(u, u_cpu), rel_l2(v, v_cpu)
    de = float(np.max(np.abs(cap.artificial_diffusivity() - eps_cpu)) / eps_cpu.max())
    print(f"fused=False against the CPU model: u {du:.3e} v {dv:.3e} eps {de:.3e}")
    assert du < _BAR and dv < _BAR and de <= _BAR


def test_every_and_the_counter():
    """``every = 4``: a launch after steps 4, 8, ...; the count runs over the attachment's life across rk4 calls; ``init`` restarts it
    and puts the physical constants back."""
    torch.cuda.set_device(0)
    case = sm.HIGH_DRIVE
    cap = pkg("shock_capture").ShockCapture(every=4)
    solver = _solver(sm.thin_box(case["ncells"], case["length"]), case["p0"], cap)
    solver.rk4(0.0, 1.0, case["dt"], max_steps=6)
    assert (cap.steps, cap.launches) == (6, 1)
    solver.rk4(6 * case["dt"], 1.0, case["dt"], max_steps=6)
    assert (cap.steps, cap.launches) == (12, 3)
    solver.init()
    assert (cap.steps, cap.launches) == (0, 0) and torch.equal(solver.cc4, solver.cc4_base) and cap.active_cells() == 0


def test_two_ranks_equal_one():
    """Two in-process ranks in lock step: the same eps per cell and the same field as one rank, to the parity bar."""
    torch.cuda.set_device(0)
    scat, utils, sc = pkg("scatterer"), pkg("utils"), pkg("shock_capture")
    case = sm.HIGH_DRIVE
    one, cap_one, (u_one, v_one, _) = _high_gpu()
    meshes = [sm.thin_box(case["ncells"], case["length"], grid=(2, 1, 1), rank=r) for r in range(2)]
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    caps = [sc.ShockCapture() for _ in meshes]
    ranks = [_solver(m, case["p0"], c, comm=scat.NativeComm(local=(7433, 2, r)), halo_plan=(od[r], gd[r]), defer_setup_exchange=True)
             for r, (m, c) in enumerate(zip(meshes, caps))]
    lockstep = pkg("solver_base").run_lockstep
    lockstep([s._setup for s in ranks])
    for s in ranks:
        s.init()
    lockstep([s.rk4_schedule(0.0, 1.0, case["dt"], max_steps=case["steps"]) for s in ranks])
    for s in ranks:
        s.check_halo_health("two ranks")
    x_one = we.centroids(one.mesh)[:, 0]
    eps_one = cap_one.artificial_diffusivity()
    lex_one = np.argsort(one.mesh.global_lexicographic_ids()[: one.mesh.nlocal])
    for s, c, m in zip(ranks, caps, meshes):
        cells = np.argmin(np.abs(we.centroids(m)[:, 0][:, None] - x_one[None, :]), axis=1)
        de = float(np.max(np.abs(c.artificial_diffusivity() - eps_one[cells])) / eps_one.max())
        lex = m.global_lexicographic_ids()[: m.nlocal]
        du, dv = rel_l2(s.u_sol(), u_one[lex_one][lex]), rel_l2(s.v_sol(), v_one[lex_one][lex])
        print(f"rank {m.rank}: {m.ncells} cells, eps {de:.3e} of max, u {du:.3e} v {dv:.3e}, launches {c.launches}")
        assert c.launches == case["steps"] and de <= _BAR and du < _BAR and dv < _BAR


def test_stable_step_covers_the_worst_case():
    """stable_time_step(1) with the attachment is no longer than without, and a step at 0.9 of it keeps the high-drive run finite with
    every loud cell forced to eps_max (s0 = -100)."""
    torch.cuda.set_device(0)
    case = sm.HIGH_DRIVE
    mesh = sm.thin_box(case["ncells"], case["length"])
    forced = pkg("shock_capture").ShockCapture(s0=-100.0)
    plain, solver = _solver(mesh, case["p0"]), _solver(mesh, case["p0"], forced)
    dt_plain, dt_cap = plain.stable_time_step(1.0), solver.stable_time_step(1.0)
    print(f"stable_time_step(1): plain {dt_plain:.6e}, with the attachment {dt_cap:.6e} (damping_max {plain.damping_max:.4e} -> "
          f"{solver.damping_max:.4e}, lambda_max {solver.lambda_max:.4e}); the case's step {case['dt']:.6e}")
    assert dt_cap <= dt_plain
    dt = 0.9 * dt_cap
    steps = int(np.ceil(case["steps"] * case["dt"] / dt))
    solver.init()
    peak = _Peak()
    solver.rk4(0.0, 1.0, dt, max_steps=steps, guard=peak)
    eps, top = forced.artificial_diffusivity(), forced.largest_diffusivity()
    loud = forced.sensor() != sm.QUIET
    print(f"forced run: {steps} steps of {dt:.4e}, overshoot {float(peak.peak.item()) / case['p0'] - 1:.4f}, loud cells {int(loud.sum())}")
    assert np.all(np.isfinite(solver.u_sol())) and np.all(np.isfinite(solver.v_sol()))
    assert loud.sum() > mesh.ncells // 2 and np.array_equal(eps[loud], top[loud]) and np.all(eps[~loud] == 0.0)
