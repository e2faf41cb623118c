"""Element receivers on the GPU: the kernel (csrc/element_receive.hpp) against numpy, receivers inside the time loops, reciprocity
between a point source and the array's elements, two in-process ranks with point sources and receivers, hipGraph replay, and time
reversal end to end through an aberrating slab."""

import numpy as np
import pytest

import point_source_cpu
from conftest import TOL, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

_lockstep = pkg("solver_base").run_lockstep
F0 = 0.5e6
T0 = 1.0 / F0


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("E", [1, 5, 300])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_element_receive_kernel(dtype, E, offset):
    """S_e = sum wgt u[dof] per element against numpy in fp64: an element without entries (writes 0), one with a single entry, one with
    5 000 (each lane strides ~20), counts that are no multiple of 64 or 256; three records into consecutive slots with two harmonics;
    two identical runs give the same bits; every operand once 256-byte aligned and once one element further."""
    import torch

    torch.cuda.set_device(0)
    ops, rec_mod = pkg("operators"), pkg("recording")
    rng = np.random.default_rng(10 * E + offset)
    counts = {1: [5000], 5: [0, 1, 5000, 63, 257]}.get(E)
    if counts is None:
        counts = [0, 1, 5000, 64, 65, 255, 256, 300, 513] + rng.integers(0, 700, E - 9).tolist()
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    K, nd = int(offs[-1]), 4000
    dof = rng.integers(0, nd, K).astype(np.int32)
    wgt = rng.uniform(0.1, 1.0, K).astype(dtype)
    us = [(rng.uniform(0.5, 2.0, nd) * rng.choice([-1.0, 1.0], nd)).astype(dtype) for _ in range(3)]
    coef = rec_mod.coefficient_rows((1, 2), 2 * np.pi * F0, [0.11 * T0, 0.47 * T0, 0.93 * T0])

    def dev(a):  # the array at an element offset into its own allocation (allocations are 256-byte aligned)
        buf = torch.zeros(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
        view = buf[offset:]
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 256 == offset * a.itemsize
        return view

    def run():
        dof_d, wgt_d, offs_d = dev(dof), dev(wgt), dev(offs)
        rec = dev(np.full(4 * E, 7.0, dtype)).view(4, E)
        hre, him = dev(np.zeros(2 * E)).view(2, E), dev(np.zeros(2 * E)).view(2, E)
        for slot, u in enumerate(us):
            ops.element_receive(dev(u), dof_d, wgt_d, offs_d, rec, slot, hre, him, dev(coef[slot]))
        torch.cuda.synchronize()
        return rec.cpu().numpy(), hre.cpu().numpy(), him.cpu().numpy()

    rec, hre, him = run()
    ref = np.array([[(wgt[offs[e]:offs[e + 1]].astype(np.float64) * u.astype(np.float64)[dof[offs[e]:offs[e + 1]]]).sum() for e in range(E)]
                    for u in us])
    tol = TOL[np.dtype(dtype)]
    assert rel_l2(rec[:3], ref) < tol["l2"] and rel_max(rec[:3], ref) < tol["mx"]
    assert np.all(rec[3] == 7.0)  # the slot after the last record is untouched
    if E > 1:
        assert np.all(rec[:3, 0] == 0.0) and np.array_equal(rec[:3, 1], np.array([wgt[0] * u[dof[0]] for u in us], dtype=dtype))
    # the harmonics accumulate the recorded (rounded) values: exact against the series, at the bar against numpy
    series = rec[:3].astype(np.float64)
    for h in range(2):
        assert np.allclose(hre[h], (series * coef[:, 2 * h][:, None]).sum(axis=0), rtol=1e-14, atol=1e-14 * np.abs(series).max())
        assert np.allclose(him[h], (series * coef[:, 2 * h + 1][:, None]).sum(axis=0), rtol=1e-14, atol=1e-14 * np.abs(series).max())
        assert rel_max(hre[h], (ref * coef[:, 2 * h][:, None]).sum(axis=0)) < 3 * tol["mx"]
    again = run()
    for a, b in zip((rec, hre, him), again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_element_receive_argument_checks():
    import torch

    torch.cuda.set_device(0)
    ops, lib_mod = pkg("operators"), pkg("_lib")
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    dof, offs = z(6, torch.int32), torch.tensor([0, 2, 6], dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        ops.element_receive(z(8), dof, z(6, torch.float32), offs)
    with pytest.raises(TypeError):
        ops.element_receive(z(8), dof.long(), z(6), offs)
    with pytest.raises(TypeError):
        ops.element_receive(z(8), dof, z(6), offs.int())
    with pytest.raises(ValueError):
        ops.element_receive(z(8), dof, z(5), offs)
    with pytest.raises(ValueError):
        ops.element_receive(z(8), dof, z(6), offs, rec=z(6).view(2, 3))
    with pytest.raises(ValueError):
        ops.element_receive(z(8), dof, z(6), offs, rec=z(4).view(2, 2), slot=2)
    with pytest.raises(ValueError):
        ops.element_receive(z(8), dof, z(6), offs, hre=z(2).view(1, 2), him=z(2).view(1, 2), coef=z(4))
    with pytest.raises(lib_mod.FusGpuError):
        ops.element_receive(z(8).cpu(), dof, z(6), offs)  # no CPU path


# ---- receivers inside the time loops -------------------------------------------------------------------------------------------------
def _small_box(P=3):
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    L = (0.008, 0.006, 0.006)
    mesh = boxmesh.BoxMesh(P, (4, 3, 3), length=L, perturb=0.1, seed=5)
    h = ls.time_step_parameters(mesh, P, 1500.0, F0, L[0])
    dt, tf, _ = ls.snap_time_step(h, P, 1500.0, F0, L[0])
    return mesh, dt, tf, pkg("sources").grid_elements(2, 2, (0.0, L[1]), (0.0, L[2]))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
def test_receivers_inside_rk4(fused):
    """The series of every step against the numpy receiver applied to ``u_sol(with_ghosts=True)`` of a second solver stepped one
    ``rk4(max_steps=1)`` at a time; ``record_from``; a full series stops recording; the harmonics are the DFT of the series; and
    receivers, sensors and a monitor given together all record."""
    import torch

    torch.cuda.set_device(0)
    ls, rx_mod, sensors, fm, rec_mod = pkg("linear_solver"), pkg("receivers"), pkg("sensors"), pkg("field_monitor"), pkg("recording")
    mesh, dt, tf, fn = _small_box()
    nsteps, E = 10, 4
    a, b = (ls.LinearSpectral3D(mesh, np.float64, fused=fused) for _ in range(2))
    rx = rx_mod.ElementReceivers(mesh, fn, np.float64, capacity=nsteps, harmonics=(1, 2), frequency=F0, n_elements=E, detJ=a.detJ_f1)
    probe = sensors.PointSensors(mesh, np.array([[0.004, 0.003, 0.003]]), np.float64, capacity=nsteps)
    mon = fm.FieldMonitor(mesh.nlocal, np.float64, peak=True)
    a.init()
    b.init()
    a.rk4(0.0, tf, dt, max_steps=nsteps, sensors=probe, monitor=mon, receivers=rx)
    assert rx.nrec == nsteps and rx.full and probe.nrec == nsteps and mon.nacc == nsteps
    bd = mesh.boundary_facets([2])
    fdm, dF = mesh.facet_dofmap(bd), a.detJ_f1.cpu().numpy()
    ref, t, times = [], 0.0, []
    for _ in range(nsteps):
        t, _ = b.rk4(t, tf, dt, max_steps=1)
        times.append(t)
        S, A = point_source_cpu.receive(b.u_sol(with_ghosts=True), rx.ids, fdm, dF, E)
        ref.append(S / A)
    ref = np.array(ref)
    series = rx.series()
    assert series.shape == (nsteps, E) and np.max(np.abs(ref)) > 0
    assert np.allclose(rx.areas(), A, rtol=1e-14)
    assert np.max(np.abs(series - ref)) < 1e-12 * np.max(np.abs(ref))
    # the harmonics: the DFT of the recorded series with the factors of recording.coefficient_rows
    coef = rec_mod.coefficient_rows((1, 2), 2 * np.pi * F0, times)
    for h, k in enumerate((1, 2)):
        dft = (series * coef[:, 2 * h][:, None]).sum(axis=0) + 1j * (series * coef[:, 2 * h + 1][:, None]).sum(axis=0)
        assert np.allclose(rx.harmonic(k), 2.0 / nsteps * dft, rtol=1e-12, atol=1e-14 * np.abs(dft).max())
    # record_from: the steps that end after it; a full series stops recording (and the run goes on)
    late = rx_mod.ElementReceivers(mesh, fn, np.float64, capacity=nsteps, n_elements=E)
    short = rx_mod.ElementReceivers(mesh, fn, np.float64, capacity=5, n_elements=E)
    for r, kw in ((late, dict(record_from=times[3])), (short, {})):
        a.init()
        _, done = a.rk4(0.0, tf, dt, max_steps=nsteps, receivers=r, **kw)
        assert done == nsteps
    assert late.nrec == 6 and not late.full and np.max(np.abs(late.series() - ref[4:])) < 1e-12 * np.max(np.abs(ref))
    assert short.nrec == 5 and short.full and np.max(np.abs(short.series() - ref[:5])) < 1e-12 * np.max(np.abs(ref))
    with pytest.raises(ValueError, match="full"):
        short.record(a.u, 0.0)


def test_graph_replay_records_receivers():
    """rk4_graph(receivers=...) without a point source: the receivers' launch follows each replay, outside the captured graph, and the
    series equals rk4's."""
    import torch

    torch.cuda.set_device(0)
    ls, rx_mod = pkg("linear_solver"), pkg("receivers")
    mesh, dt, tf, fn = _small_box()
    out = []
    for graph in (False, True):
        s = ls.LinearSpectral3D(mesh, np.float64)
        rx = rx_mod.ElementReceivers(mesh, fn, np.float64, capacity=12, n_elements=4)
        s.init()
        _, steps = (s.rk4_graph if graph else s.rk4)(0.0, tf, dt, max_steps=12, receivers=rx)
        assert steps == 12 and rx.nrec == 12
        out.append(rx.series())
    assert np.max(np.abs(out[0])) > 0 and rel_l2(out[1], out[0]) < 1e-13


# ---- reciprocity ---------------------------------------------------------------------------------------------------------------------
def test_reciprocity_between_point_and_elements():
    """Linear solver, fp64, P = 3, 6 x 4 x 4 perturbed cells, a heterogeneous speed of sound per cell (dt from the largest), uniform
    density, 2 x 2 elements, a focus strictly inside a cell, 200 steps.  Run A: a unit point source at the focus, the receivers'
    series.  Run B: element e0 alone (one-hot amplitude), a point sensor at the focus.  The lumped mass and the absorbing term are
    diagonal and K is symmetric, so  p_B(t_n) = (A_lin A_e0 / rho) r_{A,e0}(t_n),  A_lin = p0 w0 / c0; the CPU model holds this at
    1.4e-15 over 798 steps, the bar is the solvers' parity bar."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, src, rx_mod, sensors = pkg("boxmesh"), pkg("linear_solver"), pkg("sources"), pkg("receivers"), pkg("sensors")
    P, cells, L, nsteps, rho = 3, (6, 4, 4), (0.012, 0.008, 0.008), 200, 1000.0
    mesh = boxmesh.BoxMesh(P, cells, length=L, perturb=0.1, seed=11)
    c = 1500.0 * (1.0 + 0.25 * np.random.default_rng(12).uniform(-1.0, 1.0, mesh.ncells))
    h = ls.time_step_parameters(mesh, P, c.max(), F0, L[0])
    dt, _, _ = ls.snap_time_step(h, P, float(c.max()), F0, L[0])
    fn = src.grid_elements(2, 2, (0.0, L[1]), (0.0, L[2]))
    focus = np.array([[4.37 * 0.002, 2.31 * 0.002, 1.58 * 0.002]])
    kw = dict(speed_of_sound=c, density=rho, reference_speed_of_sound=1500.0)
    A = ls.LinearSpectral3D(mesh, np.float64, source_amplitude=0.0, point_source=src.PointSources(focus), **kw)
    rx = rx_mod.ElementReceivers(mesh, fn, np.float64, capacity=nsteps, n_elements=4, detJ=A.detJ_f1)
    A.init()
    A.rk4(0.0, 1.0, dt, max_steps=nsteps, receivers=rx)
    r_A, areas = rx.series(), rx.areas()
    assert r_A.shape == (nsteps, 4) and np.all(areas > 0)
    for e0 in (1, 2):
        B = ls.LinearSpectral3D(mesh, np.float64, source=src.SourceArray(fn, amplitude=np.eye(4)[e0], n_elements=4), **kw)
        probe = sensors.PointSensors(mesh, focus, np.float64, capacity=nsteps)
        B.init()
        B.rk4(0.0, 1.0, dt, max_steps=nsteps, sensors=probe)
        p_B = probe.series()[:, 0]
        want = (B.p0 * B.w0 / B.c0) * areas[e0] / rho * r_A[:, e0]
        d = rel_l2(p_B, want)
        print(f"element {e0}: max |p_B| {np.max(np.abs(p_B)):.3e}, rel l2 of the identity {d:.3e}")
        assert np.max(np.abs(p_B)) > 0 and d < 1e-11


# ---- two in-process ranks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 2, 1)], ids=["split-x", "split-y"])
def test_partitioned_points_and_receivers(grid, fused):
    """Two ranks sharing cuda:0 in this process (the mesh of tests/test_sponge_gpu.py::test_partitioned_linear_solver_with_layer).  One
    point lies exactly on the interface plane, so both ranks hold it and rank 0 alone injects it (``claim_points``); one is interior to
    rank 1; their contributions to ghost dofs travel with the stage's reverse scatter of b.  The receivers' 3 x 2 array has its middle
    row of elements cut in two by the y split; split across x, rank 1 has no receiving facet at all.  Fields against the one-rank run by
    lexicographic id, merged series against the one-rank series."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, scat, utils = pkg("boxmesh"), pkg("linear_solver"), pkg("scatterer"), pkg("utils")
    src, rx_mod, sensors = pkg("sources"), pkg("receivers"), pkg("sensors")
    P, cells, L, R, nsteps, E = 3, (4, 4, 4), 0.012, 2, 8, 6
    axis = 0 if grid[0] == 2 else 1
    pts = np.array([[0.31, 0.42, 0.37], [0.63, 0.58, 0.71]]) * L
    pts[0, axis], pts[1, axis] = 0.5 * L, 0.8 * L
    ps = src.PointSources(pts, amplitude=[0.05, 0.03], phase=[0.0, 0.9])
    fn = src.grid_elements(3, 2, (0.0, L), (0.0, L))
    meshes = [boxmesh.BoxMesh(P, cells, grid=grid, rank=r, length=L) for r in range(R)]
    serial = boxmesh.BoxMesh(P, cells, length=L)
    h = ls.time_step_parameters(serial, P, 1500.0, F0, L)
    dt, tf, _ = ls.snap_time_step(h, P, 1500.0, F0, L)
    one = ls.LinearSpectral3D(serial, np.float64, fused=fused, point_source=ps)
    rx_one = rx_mod.ElementReceivers(serial, fn, np.float64, capacity=nsteps, n_elements=E)
    free = ls.LinearSpectral3D(serial, np.float64, fused=fused)
    for s in (one, free):
        s.init()
    one.rk4(0.0, tf, dt, max_steps=nsteps, receivers=rx_one)
    free.rk4(0.0, tf, dt, max_steps=nsteps)
    u_one, v_one = one.u_sol(), one.v_sol()
    assert rel_l2(u_one, free.u_sol()) > 1e-3  # the points matter
    setups = [sensors.sensor_setup(m, pts) for m in meshes]
    assert all(0 in su.point_ids for su in setups) and 1 not in setups[0].point_ids  # both hold the interface point
    claims = src.claim_points(setups, 2)
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    wid = 8300 + 10 * grid[1] + int(fused)
    solvers = [ls.LinearSpectral3D(meshes[r], np.float64, comm=scat.NativeComm(local=(wid, R, r)), fused=fused, halo_plan=(od[r], gd[r]),
                                   defer_setup_exchange=True, point_source=ps, point_claim=claims[r]) for r in range(R)]
    assert [s._points.point_ids.tolist() for s in solvers] == [[0], [1]]  # exactly one rank claims each point
    rxs = [rx_mod.ElementReceivers(m, fn, np.float64, capacity=nsteps, n_elements=E) for m in meshes]
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        s.init()
    res = _lockstep([s.rk4_schedule(0.0, tf, dt, max_steps=nsteps, receivers=rx) for s, rx in zip(solvers, rxs)])
    torch.cuda.synchronize()
    assert all(r[1] == nsteps for r in res) and np.max(np.abs(u_one)) > 0
    for m, s in zip(meshes, solvers):
        lex = m.global_lexicographic_ids()[: m.nlocal]
        assert rel_l2(s.u_sol(), u_one[lex]) < 1e-11 and rel_l2(s.v_sol(), v_one[lex]) < 1e-11
        assert s.halo.health() == 0
    parts = [(rx.areas(), rx.integrals()) for rx in rxs]
    if axis == 1:  # the middle row of elements (ids 2, 3) is cut in two
        assert all(np.all(a[2:4] > 0) for a, _ in parts) and parts[0][0][4] == 0.0 and parts[1][0][0] == 0.0
    else:
        assert not np.any(parts[1][0]) and not np.any(parts[1][1])  # no receiving facets on rank 1: zeros, written by the kernel
    merged = rx_mod.merge(parts)
    assert np.allclose(sum(a for a, _ in parts), rx_one.areas(), rtol=1e-13)
    assert np.max(np.abs(rx_one.series())) > 0 and rel_l2(merged, rx_one.series()) < 1e-11


# ---- time reversal end to end --------------------------------------------------------------------------------------------------------
def test_time_reversal_focuses_through_an_aberrating_slab():
    """P = 4, 8 x 6 x 6 cells of 1.5 mm, f0 = 0.5 MHz, rho = 1000, c = 1500 with a slab c = 3000 (one water wavelength thick) over the
    cells with x-centroid in (2h, 4h) and y-centroid > Ly / 2: it puts the two halves of a 3 x 3 array in anti-phase at the focus
    (7.3h, Ly/2 + 0.2h, Lz/2 - 0.1h).  dt from c = 3000; 14 periods, first harmonic over the last two.  A receive run (unit point source
    at the focus, the elements' first harmonic), then three transmit runs: time-reversal phases, geometric phases (focus_phases in
    water) and zero phases.  The CPU model (oracle/rk4_oracle operators, 798 steps) gives the amplitudes 1.666e5 / 4.97e4 / 1.68e4
    against the reciprocity bound sum_e |G_e| = 1.677e5: ratios 3.35 and 9.9, 99.3 % of the bound.  The conditions below are fixed
    from that model, with room for the device's rounding, which is negligible."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, src, rx_mod, sensors = pkg("boxmesh"), pkg("linear_solver"), pkg("sources"), pkg("receivers"), pkg("sensors")
    P, cells, h, rho = 4, (8, 6, 6), 1.5e-3, 1000.0
    L = tuple(h * n for n in cells)
    mesh = boxmesh.BoxMesh(P, cells, length=L)
    cen = mesh.x_g.astype(np.float64)[mesh.x_dofs].mean(axis=1)
    c = np.where((cen[:, 0] > 2 * h) & (cen[:, 0] < 4 * h) & (cen[:, 1] > L[1] / 2), 3000.0, 1500.0)
    assert 0 < np.count_nonzero(c == 3000.0) == 2 * 3 * 6
    dt, _, _ = ls.snap_time_step(ls.time_step_parameters(mesh, P, 3000.0, F0, L[0]), P, 3000.0, F0, L[0])
    tf, t_rec = 14 * T0, 12 * T0
    fn = src.grid_elements(3, 3, (0.0, L[1]), (0.0, L[2]))
    focus = np.array([[7.3 * h, L[1] / 2 + 0.2 * h, L[2] / 2 - 0.1 * h]])
    kw = dict(speed_of_sound=c, density=rho, reference_speed_of_sound=1500.0)
    listen = ls.LinearSpectral3D(mesh, np.float64, source_amplitude=0.0, point_source=src.PointSources(focus), **kw)
    rx = rx_mod.ElementReceivers(mesh, fn, np.float64, harmonics=(1,), frequency=F0, n_elements=9, detJ=listen.detJ_f1)
    listen.init()
    _, steps = listen.rk4(0.0, tf, dt, receivers=rx, record_from=t_rec)
    R = rx.harmonic(1)
    assert np.all(np.abs(R) > 0) and rx.nacc in (2 * round(T0 / dt) - 1, 2 * round(T0 / dt), 2 * round(T0 / dt) + 1)

    def transmit(array):
        s = ls.LinearSpectral3D(mesh, np.float64, source=array, **kw)
        probe = sensors.PointSensors(mesh, focus, np.float64, harmonics=(1,), frequency=F0)
        s.init()
        s.rk4(0.0, tf, dt, sensors=probe, record_from=t_rec)
        return float(probe.harmonic_amplitude(1)[0]), s

    a_tr, s = transmit(rx_mod.time_reversal(rx))
    centres = src.grid_centres(3, 3, 0.0, (0.0, L[1]), (0.0, L[2]))
    a_geo, _ = transmit(src.SourceArray(fn, phase=src.focus_phases(centres, focus[0], 1500.0, F0), n_elements=9))
    a_flat, _ = transmit(src.SourceArray(fn, n_elements=9))
    bound = (s.p0 * s.w0 / s.c0) / rho * float(np.sum(rx.areas() * np.abs(R)))
    print(f"{steps} steps; first-harmonic amplitude at the focus: time reversal {a_tr:.4e}, geometric {a_geo:.4e}, unphased {a_flat:.4e}, "
          f"reciprocity bound {bound:.4e} (time reversal reaches {a_tr / bound:.4f} of it)")
    assert a_tr > 2 * a_geo and a_tr > 2 * a_flat
    assert a_tr >= 0.95 * bound
