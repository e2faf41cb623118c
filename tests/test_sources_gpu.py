"""Phased-array sources on the device (csrc/source_array.hpp through operators.facet_source_terms and the solvers'
``source=``): the kernel against a numpy restatement, a uniform array against the scalar source on every stage path, the
oracle's host RK4 loop with the source applied element by element, linearity, delays as time shifts, mirror symmetry of steering, and partitioned runs."""
import numpy as np
import pytest

import facet_cpu
import waveform_cpu
from conftest import pkg, rel_l2
from oracle import oracle_np, rk4_oracle

pytestmark = pytest.mark.gpu

F0, P0, C0, RHO = 0.5e6, 60000.0, 1500.0, 1000.0


_rel = facet_cpu.rel_inf  # max |a - b| / max |b|


def _dt(mesh, P, L):
    ls = pkg("linear_solver")
    h = ls.time_step_parameters(mesh, P, C0, F0, L)
    return ls.snap_time_step(h, P, C0, F0, L)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("P", [2, 3, 4, 5, 6, 7, 8])
def test_kernel_matches_numpy_restatement(P, dtype):
    import torch

    src, ops = pkg("sources"), pkg("operators")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(P)
    N, nA, nB, ndofs, E = (P + 1) ** 2, 300, 170, 5000, 23
    T = 1.0 / F0
    t, D = 14.0 * T, 12.0 * T
    # delays put s = t - tau before the start, on the ramp, on the plateau, on the ramp down and after the end of the burst
    delay = np.concatenate([[15.0 * T, 14.0 * T, 12.0 * T, 8.0 * T, 2.0 * T, 1.0 * T, 0.0], 15.0 * T * rng.random(E - 7)])
    ids = rng.integers(-1, E, nA)
    ids[:3] = -1
    tol = facet_cpu.ARRAY_TOL[np.dtype(dtype)]
    for duration in (D, None):
        for with_c2 in (True, False):
            arr = src.SourceArray(ids, amplitude=0.5 + rng.random(E), phase=2 * np.pi * rng.random(E) - np.pi, delay=delay,
                                  duration=duration, n_elements=E)
            c1, c2 = rng.random(nA).astype(dtype) + 0.5, rng.random(nA).astype(dtype) * 1e-6
            dA, dmA = rng.random((nA, N)).astype(dtype), rng.integers(0, ndofs, (nA, N)).astype(np.int32)
            xB, cB = rng.standard_normal(ndofs).astype(dtype), rng.standard_normal(nB).astype(dtype)
            dB, dmB = rng.random((nB, N)).astype(dtype), rng.integers(0, ndofs, (nB, N)).astype(np.int32)
            td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            scale = 7.0
            bound = arr.bind(None, np.zeros((nA, 2), np.int32), dtype, dev, frequency=F0, scale=scale, coeff1=td(c1),
                             coeff2=td(c2) if with_c2 else None, detJ=td(dA), dofmap=td(dmA))
            # numpy restatement, fp64 on the same (rounded) inputs
            g, dg = arr.values(t, F0, scale)
            ref = waveform_cpu.facet_reference(ndofs, g, dg, ids, c1, c2 if with_c2 else None, dA, dmA)
            refB = waveform_cpu.facet_reference(ndofs, g, dg, ids, c1, c2 if with_c2 else None, dA, dmA, (xB, cB, dB, dmB))
            assert np.max(np.abs(ref)) > 0
            stage = bound.stage_scalars(t)
            for variant in ("plain", "dev"):
                kw = dict(stage=stage) if variant == "plain" else dict(stage_dev=td(stage))
                y = torch.zeros(ndofs, dtype=bound.dtype, device=dev)
                ops.facet_source_terms(y, bound, None, **kw)
                assert _rel(y, ref) <= tol, (variant, duration, with_c2)
                y.zero_()
                ops.facet_source_terms(y, bound, (td(xB), td(cB), td(dB), td(dmB)), **kw)
                assert _rel(y, refB) <= tol, (variant, duration, with_c2)


def _uniform():
    return pkg("sources").SourceArray(lambda c: np.zeros(len(c), dtype=np.int64), n_elements=1)


@pytest.mark.parametrize("path", ["fused", "reference", "graph"])
@pytest.mark.parametrize("solver", ["linear", "westervelt"])
def test_uniform_array_equals_scalar_source(solver, path):
    import torch

    torch.cuda.set_device(0)
    boxmesh = pkg("boxmesh")
    P, L, K = 3, 0.006, 12
    mesh = boxmesh.BoxMesh(P, (4, 3, 3), length=L, perturb=0.1, seed=3)
    dt, tf, _ = _dt(mesh, P, L)
    if solver == "linear":
        mk = lambda source: pkg("linear_solver").LinearSpectral3D(mesh, np.float64, fused=path != "reference", source=source)  # noqa: E731
    else:
        mk = lambda source: pkg("nonlinear_solver").WesterveltSpectral3D(mesh, np.float64, fused=path != "reference", source=source)  # noqa: E731
    out = []
    for source in (None, _uniform()):
        s = mk(source)
        s.init()
        run = s.rk4_graph if path == "graph" else s.rk4
        _, steps = run(0.0, tf, dt, max_steps=K)
        assert steps == K
        out.append(s.u_sol())
    assert np.max(np.abs(out[0])) > 0
    assert _rel(out[1], out[0]) <= 1e-12


def _host_linear(mesh, arr, nsteps, dt):
    """The oracle's linear model (rk4_oracle.solve: its geometry, coefficients, stage and loop) with the source applied per element,
    independently of the product: mass_apply of the constant vector g_e over that element's facet rows."""
    rows = [np.nonzero(arr.assign(mesh, mesh.boundary_facets([2])) == e)[0] for e in range(arr.n_elements)]
    A = P0 * 2 * np.pi * F0 / C0

    def source_term(t, b, coefficients, detJ, dofmap):
        (fc1,) = coefficients
        g, _ = arr.values(t, F0, A)
        for e, r in enumerate(rows):
            if r.size:
                oracle_np.mass_apply(np.full(mesh.ndofs, g[e]), fc1[r], b, detJ[r], dofmap[r])

    return rk4_oracle.solve(mesh, nsteps, dt, c0=C0, rho0=RHO, f0=F0, p0=P0, source_term=source_term)[0]


def _array4(L, **kw):
    src = pkg("sources")
    return src.SourceArray(src.grid_elements(2, 2, (0.0, L), (0.0, L)), n_elements=4, **kw)


def test_linear_solver_matches_host_rk4_loop():
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    P, L, K = 2, 0.004, 40
    mesh = boxmesh.BoxMesh(P, (4, 4, 4), length=L)
    dt, _, _ = _dt(mesh, P, L)
    T = 1.0 / F0
    arr = _array4(L, amplitude=[1.0, 0.4, 0.7, 1.3], phase=[0.0, 0.9, -2.0, 3.0], delay=[0.0, 0.7 * T, 1.9 * T, 0.2 * T])
    s = ls.LinearSpectral3D(mesh, np.float64, source=arr)
    s.init()
    s.rk4(0.0, 1.0, dt, max_steps=K)
    ref = _host_linear(mesh, arr, K, dt)
    assert np.max(np.abs(ref)) > 0
    assert rel_l2(s.u_sol(), ref[: mesh.nlocal]) <= 1e-12


def test_linear_solver_is_linear_in_the_array():
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    P, L, K = 3, 0.006, 16
    mesh = boxmesh.BoxMesh(P, (4, 4, 3), length=L, perturb=0.1, seed=1)
    dt, _, _ = _dt(mesh, P, L)
    T = 1.0 / F0
    amp, tau, phi = np.array([1.0, 0.6, 1.4, 0.8]), np.array([0.0, 0.5, 1.1, 0.3]) * T, np.array([0.2, -1.0, 2.5, 0.0])

    def run(**kw):
        s = ls.LinearSpectral3D(mesh, np.float64, source=_array4(L, **kw))
        s.init()
        s.rk4(0.0, 1.0, dt, max_steps=K)
        return s.u_sol()

    u = run(amplitude=amp, phase=phi, delay=tau)
    assert np.max(np.abs(u)) > 0
    parts = [run(amplitude=np.where(np.arange(4) == e, amp, 0.0), phase=phi, delay=tau) for e in range(4)]
    assert _rel(sum(parts), u) <= 1e-12
    assert _rel(run(amplitude=amp, phase=phi + np.pi, delay=tau), -u) <= 1e-12
    u0, u90 = run(amplitude=amp, phase=0.0, delay=tau), run(amplitude=amp, phase=0.5 * np.pi, delay=tau)
    for p in (0.7, 2.9):
        assert _rel(run(amplitude=amp, phase=p, delay=tau), np.cos(p) * u0 + np.sin(p) * u90) <= 1e-12


@pytest.mark.parametrize("solver", ["linear", "westervelt"])
def test_delay_is_a_time_shift(solver):
    import torch

    torch.cuda.set_device(0)
    boxmesh = pkg("boxmesh")
    P, L, n, k = 3, 0.006, 14, 5
    mesh = boxmesh.BoxMesh(P, (4, 3, 3), length=L, perturb=0.1, seed=2)
    dt, _, _ = _dt(mesh, P, L)
    T = 1.0 / F0
    mk = (lambda a: pkg("linear_solver").LinearSpectral3D(mesh, np.float64, source=a)) if solver == "linear" else (
        lambda a: pkg("nonlinear_solver").WesterveltSpectral3D(mesh, np.float64, source=a))
    amp, phi, tau = [1.0, 0.5, 0.8, 1.2], [0.0, 1.0, 2.0, -1.0], np.array([0.0, 0.3, 0.9, 0.6]) * T
    out = []
    for shift, steps in ((0.0, n), (k * dt, n + k)):
        s = mk(_array4(L, amplitude=amp, phase=phi, delay=tau + shift))
        s.init()
        s.rk4(0.0, 1.0, dt, max_steps=steps)
        out.append(s.u_sol())
    assert np.max(np.abs(out[0])) > 0
    assert _rel(out[1], out[0]) <= 1e-11


def test_steering_mirrors_under_y_reflection():
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, src = pkg("boxmesh"), pkg("linear_solver"), pkg("sources")
    P, L, K = 3, 0.006, 20
    mesh = boxmesh.BoxMesh(P, (4, 4, 2), length=L)
    dt, _, _ = _dt(mesh, P, L)
    fn = src.grid_elements(4, 1, (0.0, L), (0.0, L))
    centres = src.grid_centres(4, 1, 0.0, (0.0, L), (0.0, L))
    th = 0.35
    fields = []
    for sgn in (1.0, -1.0):
        arr = src.SourceArray(fn, delay=src.steer_delays(centres, [np.cos(th), sgn * np.sin(th), 0.0], C0), n_elements=4)
        s = ls.LinearSpectral3D(mesh, np.float64, source=arr)
        s.init()
        s.rk4(0.0, 1.0, dt, max_steps=K)
        fields.append(s.u_sol())
    up, um = fields
    x = mesh.dof_coordinates()[: mesh.nlocal]
    key = lambda p: np.round(p / L * 1e9).astype(np.int64)  # noqa: E731
    lookup = {tuple(r): i for i, r in enumerate(key(x))}
    mirror = np.array([lookup[tuple(r)] for r in key(x * [1, -1, 1] + [0, L, 0])])
    assert np.max(np.abs(up)) > 0 and _rel(up, up[mirror]) > 1e-3  # steering breaks the symmetry of each field ...
    assert _rel(um[mirror], up) <= 1e-11  # ... and the mirrored steering mirrors it


_lockstep = pkg("solver_base").run_lockstep


@pytest.mark.parametrize("grid", [(1, 2, 1), (1, 2, 2)], ids=["2ranks", "4ranks"])
def test_partitioned_array_equals_single_rank(grid):
    """2 / 4 ranks sharing cuda:0 in this process (in-process transport), each binding its own source facets by centroid:
    the owned dofs equal the single-rank run."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, scat, utils = pkg("boxmesh"), pkg("linear_solver"), pkg("scatterer"), pkg("utils")
    P, cells, L, K = 3, (4, 4, 4), 0.006, 10
    R = int(np.prod(grid))
    T = 1.0 / F0
    kw = dict(amplitude=[1.0, 0.5, 0.8, 1.2], phase=[0.0, 1.0, 2.0, -1.0], delay=np.array([0.0, 0.3, 0.9, 0.6]) * T)
    serial = boxmesh.BoxMesh(P, cells, length=L)
    dt, _, _ = _dt(serial, P, L)
    one = ls.LinearSpectral3D(serial, np.float64, source=_array4(L, **kw))
    one.init()
    one.rk4(0.0, 1.0, dt, max_steps=K)
    ref = np.empty(serial.ndofs_global)
    ref[serial.global_lexicographic_ids()[: serial.nlocal]] = one.u_sol()
    meshes = [boxmesh.BoxMesh(P, cells, grid=grid, rank=r, length=L, ghost_order=5) for r in range(R)]
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    wid = 7700 + 10 * R
    solvers = [ls.LinearSpectral3D(meshes[r], np.float64, comm=scat.NativeComm(local=(wid, R, r)), halo_plan=(od[r], gd[r]),
                                   defer_setup_exchange=True, source=_array4(L, **kw)) for r in range(R)]
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        s.init()
    res = _lockstep([s.rk4_schedule(0.0, 1.0, dt, K) for s in solvers])
    torch.cuda.synchronize()
    for s in solvers:
        s.check_halo_health("test")
    assert all(r[1] == K for r in res)
    assert sum(s.source.nfacets for s in solvers) == one.source.nfacets and all(s.source.nfacets > 0 for s in solvers)
    for m, s in zip(meshes, solvers):
        mine = ref[m.global_lexicographic_ids()[: m.nlocal]]
        assert np.max(np.abs(s.u_sol() - mine)) <= 1e-11 * np.max(np.abs(ref))


def test_linear_box_demo_array_reports_the_peak():
    import os
    import subprocess
    import sys

    from conftest import ROOT

    r = subprocess.run([sys.executable, os.path.join(ROOT, "fenicsx-fus-gpu_amd", "demo_linear_box.py"), "--cells", "6", "--degree", "2",
                        "--max-steps", "30", "--array", "2,3", "--focus", "0.03,0.06,0.05"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Solve time per step" in r.stdout, r.stdout + r.stderr
    got = {ln.split(":")[0]: ln.split(":", 1)[1] for ln in r.stdout.splitlines() if ln.startswith(("Peak", "Array"))}
    assert got["Array elements"].startswith(" 2 x 3, focus: (0.03, 0.06, 0.05)")
    assert float(got["Peak pressure at the focus"]) > 0.0 and float(got["Peak pressure on the axis"].split(" at ")[0]) > 0.0
