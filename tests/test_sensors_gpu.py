"""Point sensors on the device (csrc/probe.hpp through sensors.PointSensors): evaluation against the host's
``point_evaluation.eval_function``, the accumulators against numpy, the solvers' ``rk4(..., sensors=...)`` (fused path,
reference sequence, hipGraph replay, 2 / 4 in-process ranks) and the two demos' sensor options."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg
from oracle import rk4_oracle

pytestmark = pytest.mark.gpu

# every degree probe_eval_kernel is compiled for (tests/test_cell_model64.py compares this list with the compiled names)
DEGREES = list(range(1, 11))


def _bowl(L, N):
    def warp(xg):
        out = xg.copy()
        yy, zz = xg[:, 1] / L - 0.5, xg[:, 2] / L - 0.5
        out[:, 0] = xg[:, 0] + 0.15 * (L / N) * 4 * (yy * yy + zz * zz) * (1.0 - xg[:, 0] / L)
        return out

    return warp


def _mesh(kind, P, L=0.012, cells=(3, 2, 2)):
    boxmesh = pkg("boxmesh")
    if kind == "affine":
        return boxmesh.BoxMesh(P, cells, length=L)
    if kind == "perturbed":
        return boxmesh.BoxMesh(P, cells, length=L, perturb=0.14, seed=2)
    if kind == "bowl":
        return boxmesh.BoxMesh(P, cells, length=L, warp=_bowl(L, cells[0]))
    ad = pkg("dolfinx_adaptor")  # "array": cells and vertices renumbered at random
    box = boxmesh.BoxMesh(P, cells, length=L, perturb=0.1, seed=4)
    rng = np.random.default_rng(7)
    cperm, vperm = rng.permutation(box.ncells), rng.permutation(box.x_g.shape[0])
    vinv = np.empty_like(vperm)
    vinv[vperm] = np.arange(vperm.size)
    return ad.ArrayMesh(P, box.dofmap[cperm], vinv[box.x_dofs[cperm]], box.x_g[vperm])


def _points(mesh, L, rng, m=120):
    """Interior random points, the interior cell corners, and (affine) points on the domain boundary."""
    pts = 0.1 * L + 0.8 * L * rng.random((m, 3))
    xg = np.asarray(mesh.x_g, dtype=np.float64)
    corners = xg[np.all((xg > 0.05 * L) & (xg < 0.95 * L), axis=1)]
    boundary = np.array([[0, 0, 0], [L, L, L], [0.0, 0.5 * L, 0.3 * L], [L, 0.2 * L, 0.9 * L], [0.4 * L, L, 0.0]])
    return np.concatenate([pts, corners] + ([boundary] if isinstance(mesh, pkg("boxmesh").BoxMesh) and mesh.x_g.min() == 0 else []))


def _rel(a, b):
    a, b = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x, dtype=np.float64) for x in (a, b))
    assert a.shape == b.shape
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if a.size else 0.0


def _dev(a, dt):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["affine", "perturbed", "bowl", "array"])
@pytest.mark.parametrize("P", DEGREES)
def test_device_evaluation_matches_eval_function(P, kind, dtype):
    import torch

    torch.cuda.set_device(0)
    pe, sens = pkg("point_evaluation"), pkg("sensors")
    L = 0.012
    mesh = _mesh(kind, P, L)
    rng = np.random.default_rng(P)
    pts = _points(mesh, L, rng)
    u = (1e4 * rng.standard_normal(mesh.ndofs)).astype(dtype)
    s = sens.PointSensors(mesh, pts, dtype)
    got = s.evaluate(_dev(u, dtype)).cpu().numpy()
    assert got.dtype == dtype and got.shape == (s.point_ids.size,)
    ref = pe.eval_function(mesh, u.astype(np.float64), s.points, s.setup.cells)
    tol = 1e-13 if dtype == np.float64 else 1e-5
    assert np.max(np.abs(got - ref)) <= tol * np.max(np.abs(ref))
    # the same values through compute_eval_params in the caller's point order
    x_eval, cell_eval = pe.compute_eval_params(mesh, pts.T)
    order = np.argsort(s.point_ids)
    assert np.array_equal(s.points[order], x_eval)
    assert np.max(np.abs(got[order] - pe.eval_function(mesh, u.astype(np.float64), x_eval, cell_eval))) <= tol * np.max(np.abs(ref))


def test_empty_and_single_point_sets():
    import torch

    torch.cuda.set_device(0)
    pe, sens = pkg("point_evaluation"), pkg("sensors")
    mesh = _mesh("perturbed", 4)
    u = np.random.default_rng(0).standard_normal(mesh.ndofs)
    ud = _dev(u, np.float64)
    empty = sens.PointSensors(mesh, np.zeros((0, 3)), np.float64, capacity=3, peak=True, harmonics=(1,), frequency=1e6)
    assert empty.evaluate(ud).numel() == 0
    empty.record(ud, 0.1)
    assert empty.series().shape == (1, 0) and empty.peak()[0].shape == (0,)
    outside = sens.PointSensors(mesh, [[1.0, 1.0, 1.0]], np.float64)
    assert outside.point_ids.size == 0 and outside.evaluate(ud).numel() == 0
    one = sens.PointSensors(mesh, [0.005, 0.004, 0.007], np.float64)
    assert one.point_ids.tolist() == [0]
    ref = pe.eval_function(mesh, u, one.points, one.setup.cells)
    assert abs(one.evaluate(ud).item() - ref[0]) <= 1e-13 * max(1.0, abs(ref[0]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_accumulators_against_numpy(dtype):
    """Series rows = evaluate() of each field; peaks = the extrema of the series, bitwise; harmonics exact on
    p = A1 cos(w t + phi1) + A2 cos(2 w t + phi2) + c sampled at N equal steps over one period."""
    import torch

    torch.cuda.set_device(0)
    sens = pkg("sensors")
    P, L = 4, 0.012
    mesh = _mesh("bowl", P, L)
    rng = np.random.default_rng(11)
    pts = _points(mesh, L, rng, m=300)
    K = 9
    s = sens.PointSensors(mesh, pts, dtype, capacity=K, peak=True)
    fields = [(1e3 * rng.standard_normal(mesh.ndofs)).astype(dtype) for _ in range(K)]
    rows = []
    for k, f in enumerate(fields):
        fd = _dev(f, dtype)
        rows.append(s.evaluate(fd).cpu().numpy())
        s.record(fd, k * 1e-7)
    assert s.full
    with pytest.raises(ValueError):
        s.record(fd, 1.0)
    series = s.series()
    assert series.dtype == dtype and np.array_equal(series, np.asarray(rows))
    pmax, pmin = s.peak()
    assert np.array_equal(pmax, series.max(axis=0).astype(np.float64)) and np.array_equal(pmin, series.min(axis=0).astype(np.float64))
    s.reset()
    assert s.nrec == 0 and np.all(s.peak()[0] == -np.inf)

    f0, N = 1.1e6, 24
    w = 2 * np.pi * f0
    h = sens.PointSensors(mesh, pts, dtype, peak=True, harmonics=(1, 2, 3), frequency=f0)
    g1, g2 = rng.standard_normal(mesh.ndofs), rng.standard_normal(mesh.ndofs)
    a1, a2 = h.evaluate(_dev(g1, dtype)).cpu().numpy(), h.evaluate(_dev(g2, dtype)).cpu().numpy()
    for k in range(N):
        t = 5e-6 + (k + 1) / (N * f0)
        field = 3.0 * g1 * np.cos(w * t + 0.4) + 0.5 * g2 * np.cos(2 * w * t - 1.0) + 0.25
        h.record(_dev(field, dtype), t)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert np.max(np.abs(h.harmonic_amplitude(1) - 3.0 * np.abs(a1))) <= tol * 3 * np.max(np.abs(a1))
    assert np.max(np.abs(h.harmonic_amplitude(2) - 0.5 * np.abs(a2))) <= tol * 3 * np.max(np.abs(a1))
    assert np.max(h.harmonic_amplitude(3)) <= tol * 3 * np.max(np.abs(a1))


def test_planned_and_ring_records_accumulate_alike():
    """80 records of which only the first 10 are planned (expect_steps): those read the uploaded table, the other 70 = _RING + 6
    the pinned ring, whose first six rows are reused after the wrap.  Harmonics and peaks against numpy over the per-record
    evaluate() rows."""
    import torch

    torch.cuda.set_device(0)
    sens, rec = pkg("sensors"), pkg("recording")
    mesh = _mesh("perturbed", 2)
    rng = np.random.default_rng(29)
    K, f0, dt = 10 + rec._RING + 6, 1.1e6, 0.9e-7 / 7
    s = sens.PointSensors(mesh, 0.001 + 0.01 * rng.random((40, 3)), np.float64, peak=True, harmonics=(1, 2), frequency=f0)
    assert s.m == 40
    ends = rec.record_times(0.0, 1.0, dt, max_steps=K)
    s.expect_steps(0.0, 1.0, dt, max_steps=10)  # a run whose step ends are t_0 .. t_9
    assert np.array_equal(s.factors.planned_times, ends[:10])
    rows = []
    for k in range(K):
        fd = _dev(1e3 * rng.standard_normal(mesh.ndofs), np.float64)
        rows.append(s.evaluate(fd).cpu().numpy())
        s.record(fd, ends[k])
        assert s.factors.planned_left == max(9 - k, 0)
    rows = np.asarray(rows)  # [K, m]
    assert s.nacc == K and s.nrec == 0
    pmax, pmin = s.peak()
    assert np.array_equal(pmax, rows.max(axis=0)) and np.array_equal(pmin, rows.min(axis=0))
    for k in (1, 2):
        ph = k * 2 * np.pi * f0 * np.asarray(ends)
        amp = 2.0 / K * np.hypot(rows.T @ np.cos(ph), rows.T @ -np.sin(ph))
        assert np.max(amp) > 0 and np.max(np.abs(s.harmonic_amplitude(k) - amp)) <= 1e-10 * np.max(amp)


def _linear(mesh, fused, P, L):
    ls = pkg("linear_solver")
    h = ls.time_step_parameters(mesh, P, 1500.0, 0.5e6, L)
    dt, tf, _ = ls.snap_time_step(h, P, 1500.0, 0.5e6, L)
    s = ls.LinearSpectral3D(mesh, np.float64, fused=fused)
    s.init()
    return s, dt, tf


def _westervelt(mesh, fused, P, L):
    ls, nls = pkg("linear_solver"), pkg("nonlinear_solver")
    h = ls.time_step_parameters(mesh, P, 1480.0, 1.1e6, L)
    dt, tf, _ = ls.snap_time_step(h, P, 1480.0, 1.1e6, L)
    s = nls.WesterveltSpectral3D(mesh, np.float64, fused=fused)
    s.init()
    return s, dt, tf


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
@pytest.mark.parametrize("solver", ["linear", "westervelt"])
def test_solver_records_every_step(solver, fused):
    """rk4(..., sensors=s) over K steps: the rows equal eval_function of u_sol() after the same number of
    rk4(max_steps=1) calls; the solution is the one of rk4 without sensors; record_from skips early steps.  Separate runs are
    compared to rounding: the cell kernels add with float atomics, whose order varies from run to run."""
    import torch

    torch.cuda.set_device(0)
    pe, sens = pkg("point_evaluation"), pkg("sensors")
    P, L, K = 4, 0.006, 6
    mesh = pkg("boxmesh").BoxMesh(P, (4, 3, 3), length=L, warp=_bowl(L, 4))
    make = _linear if solver == "linear" else _westervelt
    pts = _points(mesh, L, np.random.default_rng(3), m=80)
    a, dt, tf = make(mesh, fused, P, L)
    s = sens.PointSensors(mesh, pts, np.float64, capacity=K, harmonics=(1, 2), frequency=a.f0)
    t, steps = a.rk4(0.0, tf, dt, max_steps=K, sensors=s)
    assert steps == K and s.nrec == K
    # the harmonic factors the solver uploaded for its step-end times, against the series
    ends, te = [], 0.0
    for _ in range(K):
        te += dt
        ends.append(te)
    for k in (1, 2):
        ph = k * 2 * np.pi * a.f0 * np.asarray(ends)
        acc = s.series().T @ np.stack([np.cos(ph), -np.sin(ph)], axis=1)
        assert _rel(s.harmonic_amplitude(k), 2.0 / K * np.hypot(acc[:, 0], acc[:, 1])) < 1e-12
    b, _, _ = make(mesh, fused, P, L)
    tb, ref = 0.0, []
    for _ in range(K):
        tb, _ = b.rk4(tb, tf, dt, max_steps=1)
        ref.append(pe.eval_function(mesh, b.u_sol(), s.points, s.setup.cells))
    ref = np.asarray(ref)
    assert np.max(np.abs(ref)) > 0
    assert np.max(np.abs(s.series() - ref)) <= 1e-12 * np.max(np.abs(ref))
    c, _, _ = make(mesh, fused, P, L)
    c.rk4(0.0, tf, dt, max_steps=K)
    assert _rel(a.u, c.u) < 1e-13 and _rel(a.v, c.v) < 1e-13
    d, _, _ = make(mesh, fused, P, L)
    late = sens.PointSensors(mesh, pts, np.float64, capacity=K)
    d.rk4(0.0, tf, dt, max_steps=K, sensors=late, record_from=3.5 * dt)
    assert late.nrec == K - 3 and _rel(late.series(), s.series()[3:]) < 1e-13
    small = sens.PointSensors(mesh, pts, np.float64, capacity=2)  # a full series stops recording, not the run
    e, _, _ = make(mesh, fused, P, L)
    assert e.rk4(0.0, tf, dt, max_steps=K, sensors=small)[1] == K
    assert _rel(small.series(), s.series()[:2]) < 1e-13


@pytest.mark.parametrize("solver", ["linear", "westervelt"])
def test_graph_replay_records_like_rk4(solver):
    import torch

    torch.cuda.set_device(0)
    sens = pkg("sensors")
    P, L, K = 3, 0.006, 7
    mesh = pkg("boxmesh").BoxMesh(P, (4, 3, 3), length=L, perturb=0.1, seed=1)
    make = _linear if solver == "linear" else _westervelt
    pts = _points(mesh, L, np.random.default_rng(5), m=60)
    a, dt, tf = make(mesh, True, P, L)
    sa = sens.PointSensors(mesh, pts, np.float64, capacity=K, peak=True, harmonics=(1,), frequency=a.f0)
    a.rk4(0.0, tf, dt, max_steps=K, sensors=sa, record_from=1.5 * dt)
    b, _, _ = make(mesh, True, P, L)
    sb = sens.PointSensors(mesh, pts, np.float64, capacity=K, peak=True, harmonics=(1,), frequency=b.f0)
    assert b.rk4_graph(0.0, tf, dt, max_steps=K, sensors=sb, record_from=1.5 * dt)[1] == K
    assert sa.nrec == sb.nrec == K - 1
    assert _rel(sa.series(), sb.series()) < 1e-13  # two runs: equal to the rounding of the cell kernels' float atomics
    assert _rel(sa.peak()[0], sb.peak()[0]) < 1e-13 and _rel(sa.harmonic_amplitude(1), sb.harmonic_amplitude(1)) < 1e-12
    assert _rel(a.u, b.u) < 1e-13


_lockstep = pkg("solver_base").run_lockstep


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 1)], ids=["2ranks", "4ranks"])
def test_partitioned_series_equal_the_single_rank_series(grid, fused):
    """2 / 4 ranks sharing cuda:0 in this process (in-process transport): each rank records the points in its cells after a
    forward exchange of the field; merged over the ranks the series equal the single-rank series."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, scat, utils, sens = pkg("boxmesh"), pkg("linear_solver"), pkg("scatterer"), pkg("utils"), pkg("sensors")
    P, cells, L, K = 3, (4, 4, 4), 0.012, 6
    R = int(np.prod(grid))
    meshes = [boxmesh.BoxMesh(P, cells, grid=grid, rank=r, length=L, ghost_order=5) for r in range(R)]
    serial = boxmesh.BoxMesh(P, cells, length=L)
    rng = np.random.default_rng(9)
    pts = np.concatenate([L * rng.random((150, 3)), [[0.5 * L, 0.5 * L, 0.5 * L], [0.5 * L, 0.3 * L, 0.7 * L], [0.25 * L, 0.5 * L, 0.1 * L]]])
    h = ls.time_step_parameters(serial, P, 1500.0, 0.5e6, L)
    dt, tf, _ = ls.snap_time_step(h, P, 1500.0, 0.5e6, L)
    one = ls.LinearSpectral3D(serial, np.float64, fused=fused)
    one.init()
    s1 = sens.PointSensors(serial, pts, np.float64, capacity=K)
    one.rk4(0.0, tf, dt, max_steps=K, sensors=s1)
    ref = sens.merge([(s1.point_ids, s1.series())], pts.shape[0])
    assert not np.isnan(ref).any() and np.max(np.abs(ref)) > 0
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    wid = 7600 + 10 * R + int(fused)
    solvers = [ls.LinearSpectral3D(meshes[r], np.float64, comm=scat.NativeComm(local=(wid, R, r)), fused=fused,
                                   halo_plan=(od[r], gd[r]), defer_setup_exchange=True) for r in range(R)]
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        s.init()
    sensors = [sens.PointSensors(m, pts, np.float64, capacity=K) for m in meshes]
    res = _lockstep([s.rk4_schedule(0.0, tf, dt, K, sensors=se) for s, se in zip(solvers, sensors)])
    torch.cuda.synchronize()
    for s in solvers:
        s.check_halo_health("test")
    assert all(r[1] == K for r in res) and all(se.nrec == K for se in sensors)
    merged = sens.merge([(se.point_ids, se.series()) for se in sensors], pts.shape[0])
    assert np.max(np.abs(merged - ref)) <= 1e-11 * np.max(np.abs(ref))


def test_bowl_demo_sensor_plane_records_one_period(tmp_path, oracle_c):
    """demo_nonlinear_bowl.py --sensor-plane: the last period recorded in ONE rk4 call; one file per step of the period; the
    last equals eval_function of the oracle-side Westervelt loop at the same points to the file's 8 decimals."""
    pe, boxmesh, ls = pkg("point_evaluation"), pkg("boxmesh"), pkg("linear_solver")
    out_dir, peak = os.path.join(tmp_path, "fields"), os.path.join(tmp_path, "peak.txt")
    P, N, L = 3, 4, 0.004
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fenicsx-fus-gpu_amd", "demo_nonlinear_bowl.py"), "--degree", str(P), "--cells", str(N),
                        "--length", str(L), "--out-dir", out_dir, "--sensor-plane", "9,7", "--peak-out", peak],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Solve time per step" in r.stdout, r.stdout + r.stderr
    lines = {ln.split(":")[0]: ln.split(":")[1].strip() for ln in r.stdout.splitlines() if ln.startswith("Number of")}
    spp = int(lines["Number of steps per period"])
    files = sorted(os.listdir(out_dir), key=lambda f: int(f.split("_")[-1][:-4]))
    assert files == [f"pressure_field_{k}.txt" for k in range(spp)]
    last = np.loadtxt(os.path.join(out_dir, files[-1]), delimiter=",")
    assert 40 < last.shape[0] <= 63 and last.shape[1] == 3  # the bowl's curved face leaves some grid points outside
    mesh = boxmesh.BoxMesh(P, N, length=L, warp=_bowl(L, N))
    c0, f0 = 1480.0, 1.1e6
    h = ls.time_step_parameters(mesh, P, c0, f0, L)
    dt = (1 / f0) / spp
    first = int(np.floor((L / c0 + 6.0 / f0) / dt)) + 1
    while not first * dt > L / c0 + 6.0 / f0:
        first += 1
    k_last = first + spp - 1
    u_ref, _ = rk4_oracle.solve_westervelt(mesh, k_last, dt, c0=c0, f0=f0, oracle_c=oracle_c)
    # the demo's grid (the file's coordinates are rounded to 8 decimals: evaluate at the exact points)
    X, Y = np.meshgrid(np.linspace(0.0, L, 9), np.linspace(0.0, L, 7), indexing="ij")
    pts = np.stack([X.reshape(-1), Y.reshape(-1), np.full(X.size, 0.5 * L)], axis=1)
    x_eval, cell_eval = pe.compute_eval_params(mesh, pts.T)
    assert len(cell_eval) == last.shape[0] and np.max(np.abs(x_eval[:, :2] - last[:, :2])) < 1e-8
    ref = pe.eval_function(mesh, u_ref, x_eval, cell_eval)
    assert np.max(np.abs(ref)) > 1.0
    assert np.max(np.abs(last[:, 2] - ref)) < 1e-7 + 1e-9 * np.max(np.abs(ref))
    pk = np.loadtxt(peak, delimiter=",")
    allf = np.stack([np.loadtxt(os.path.join(out_dir, f), delimiter=",")[:, 2] for f in files])
    assert pk.shape == (last.shape[0], 6) and np.allclose(pk[:, :2], last[:, :2])
    assert np.all(pk[:, 2] >= allf.max(axis=0) - 1e-8) and np.all(pk[:, 3] <= allf.min(axis=0) + 1e-8)
    assert np.max(pk[:, 4]) > 0 and np.all(pk[:, 4] >= 0) and np.all(pk[:, 5] >= 0)


def test_linear_box_demo_device_eval_matches_host_eval(tmp_path):
    pkgdir = os.path.join(ROOT, "fenicsx-fus-gpu_amd")
    out = []
    for extra in ([], ["--device-eval"]):
        ev = os.path.join(tmp_path, "dev" if extra else "host")
        r = subprocess.run([sys.executable, os.path.join(pkgdir, "demo_linear_box.py"), "--cells", "6", "--degree", "3",
                            "--max-steps", "5", "--eval-out", ev] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Solve time per step" in r.stdout, r.stdout + r.stderr
        out.append(np.loadtxt(os.path.join(ev, "pressure_field_nproc1.txt"), delimiter=","))
    host, dev = out
    assert host.shape == dev.shape == (10000, 3) and np.max(np.abs(host[:, 2])) > 0
    assert np.array_equal(host[:, :2], dev[:, :2]) and np.max(np.abs(host[:, 2] - dev[:, 2])) <= 1.5e-8
