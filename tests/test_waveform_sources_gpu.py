"""Sampled source waveforms on the GPU (csrc/source_wave.hpp through operators.facet_source_terms / point_source_terms and the solvers'
``source=`` / ``point_source=``): the two kernels against their numpy restatement, a sampled analytic source against the analytic one
in every solver form, the solvers against the CPU model for a pulse no analytic source represents, hipGraph replay, a partitioned
run, and time reversal of the recorded signals end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import point_source_cpu
import waveform_cpu
from conftest import ROOT, TOL, pkg, rel_l2, rel_max
from oracle import rk4_oracle

pytestmark = pytest.mark.gpu

F0, P0, C0 = 0.5e6, 60000.0, 1500.0
T0 = 1.0 / F0
# every degree point_source_wave_kernel is compiled for (tests/test_cell_model64.py compares this list with the compiled names); the
# facet kernel's test runs the same list
DEGREES = list(range(1, 11))
_lockstep = pkg("solver_base").run_lockstep

# the table of the kernel tests: a power-of-two interval, so that node times and (s - t0) / dt are exact
DT_TAB, T0_TAB, T_STAGE = 2.0**-24, 5 * 2.0**-24, 40 * 2.0**-24


def _time_cases(nt):
    """s - t0 in units of dt for: before the table, exactly on its first node, inside an interval, exactly on an interior node,
    exactly on the last node, past the end (and, for a table of more than two samples, inside the last interval)."""
    return np.array([-2.0, 0.0, 0.3 if nt == 2 else 7.3, 0.5 if nt == 2 else 11.0, nt - 1.0, nt - 0.5, nt - 1.25])


def _delays(nt, count):
    """``count`` delays that put s = T_STAGE - tau on the cases of ``_time_cases``, in turn."""
    x = _time_cases(nt)
    return T_STAGE - (T0_TAB + x[np.arange(count) % x.size] * DT_TAB)


def _random_table(rng, rows, nt):
    return pkg("sources").SampledWaveform(rng.standard_normal((rows, nt)), DT_TAB, t0=T0_TAB, derivative=rng.standard_normal((rows, nt)) / DT_TAB)


def _dt(mesh, P, L, c=C0, f0=F0):
    ls = pkg("linear_solver")
    return ls.snap_time_step(ls.time_step_parameters(mesh, P, c, f0, L), P, c, f0, L)


# ---- 8. the facet kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [33, 2], ids=["Nt33", "Nt2"])
@pytest.mark.parametrize("rows", ["R1", "RE"])
@pytest.mark.parametrize("P", DEGREES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_facet_wave_kernel(dtype, P, rows, nt):
    """The nine source facets of a 3 x 3 x 3 box: eight elements and one inactive facet; element 6 is mapped to row -1; the delays of
    elements 0 .. 5 put them, in ONE launch, before the table, exactly on its first node, inside an interval, exactly on an interior
    node, exactly on the last node and past the end (element 7: inside the last interval).  With and without cA2, with and without set
    B, host stage and device stage, against the numpy restatement in fp64."""
    import torch

    torch.cuda.set_device(0)
    src, ops, boxmesh = pkg("sources"), pkg("operators"), pkg("boxmesh")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(100 * P + nt)
    mesh = boxmesh.BoxMesh(P, (3, 3, 3), length=0.003)
    bd = mesh.boundary_facets([2])
    assert bd.shape[0] == 9
    N, ndofs, E, nB = (P + 1) ** 2, mesh.ndofs, 8, 170
    ids = np.array([0, 1, 2, 3, -1, 4, 5, 6, 7])
    wf = _random_table(rng, 1 if rows == "R1" else E, nt)
    row_of = np.array([0, 0, 0, 0, 0, 0, -1, 0]) if rows == "R1" else np.array([3, 1, 0, 2, 5, 4, -1, 7])
    delay = np.append(_delays(nt, 7)[[0, 1, 2, 3, 4, 5, 0]], _delays(nt, 7)[6])
    arr = src.SourceArray(ids, amplitude=0.5 + rng.random(E), delay=delay, waveform=wf, waveform_of_element=row_of)
    scale = 7.0
    g, dg = arr.values(T_STAGE, F0, scale)
    live = [1, 2, 3, 4, 7]
    assert np.all(g[live] != 0.0) and not np.any(g[[0, 5, 6]]) and not np.any(dg[[0, 5, 6]])
    assert g[1] == arr.amplitude[1] * scale * wf.samples[row_of[1], 0] and g[4] == arr.amplitude[4] * scale * wf.samples[row_of[4], -1]
    assert g[3] == arr.amplitude[3] * scale * wf.samples[row_of[3], 0 if nt == 2 else 11] or nt == 2
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dmA = np.asarray(mesh.facet_dofmap(bd), dtype=np.int32).reshape(9, N)
    c1, c2, dA = rng.random(9).astype(dtype) + 0.5, (rng.random(9) * DT_TAB).astype(dtype), rng.random((9, N)).astype(dtype)
    xB, cB = rng.standard_normal(ndofs).astype(dtype), rng.standard_normal(nB).astype(dtype)
    dB, dmB = rng.random((nB, N)).astype(dtype), rng.integers(0, ndofs, (nB, N)).astype(np.int32)
    tol = TOL[np.dtype(dtype)]
    for with_c2 in (True, False):
        bound = arr.bind(mesh, bd, dtype, dev, frequency=F0, scale=scale, coeff1=td(c1), coeff2=td(c2) if with_c2 else None, detJ=td(dA),
                         dofmap=td(dmA))
        assert bound.table.dtype == torch.float64 and tuple(bound.table.shape) == ((1 if rows == "R1" else 7), nt, 2)
        assert bound.row_of_element.dtype == torch.int32 and int(bound.row_of_element[6]) == -1
        ref = waveform_cpu.facet_reference(ndofs, g, dg, ids, c1, c2 if with_c2 else None, dA, dmA)
        refB = waveform_cpu.facet_reference(ndofs, g, dg, ids, c1, c2 if with_c2 else None, dA, dmA, (xB, cB, dB, dmB))
        assert np.max(np.abs(ref)) > 0
        stage = bound.stage_scalars(T_STAGE)
        for variant in ("plain", "dev"):
            kw = dict(stage=stage) if variant == "plain" else dict(stage_dev=td(stage))
            y = torch.zeros(ndofs, dtype=bound.dtype, device=dev)
            ops.facet_source_terms(y, bound, None, **kw)
            got = y.cpu().numpy()
            print(f"{variant} c2 {with_c2}: rel l2 {rel_l2(got, ref):.3e} max {rel_max(got, ref):.3e}")
            assert rel_l2(got, ref) < tol["l2"] and rel_max(got, ref) < tol["mx"], (variant, with_c2)
            # facets of silent, inactive and out-of-table elements issue no atomic: their dofs keep their zero bits
            quiet = np.setdiff1d(dmA[np.isin(ids, [0, 5, 6, -1])].reshape(-1), dmA[np.isin(ids, live)].reshape(-1))
            assert quiet.size and not np.any(got[quiet])
            y.zero_()
            ops.facet_source_terms(y, bound, (td(xB), td(cB), td(dB), td(dmB)), **kw)
            got = y.cpu().numpy()
            assert rel_l2(got, refB) < tol["l2"] and rel_max(got, refB) < tol["mx"], (variant, with_c2, "set B")


def test_facet_source_terms_checks_the_table():
    import torch

    torch.cuda.set_device(0)
    src, ops, boxmesh = pkg("sources"), pkg("operators"), pkg("boxmesh")
    dev = torch.device("cuda", 0)
    mesh = boxmesh.BoxMesh(2, (2, 2, 2), length=0.002)
    bd = mesh.boundary_facets([2])
    wf = _random_table(np.random.default_rng(0), 4, 9)
    arr = src.SourceArray([0, 1, 2, 3], waveform=wf)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    mk = lambda: arr.bind(mesh, bd, np.float64, dev, frequency=F0, scale=1.0, coeff1=z(4), detJ=z(4, 9), dofmap=z(4, 9, dt=torch.int32))  # noqa: E731
    y = z(mesh.ndofs)
    ops.facet_source_terms(y, mk(), None, stage=np.zeros(6))
    for change, err in ((dict(table=z(4, 9, 2, dt=torch.float32)), TypeError), (dict(table=z(4, 8, 2)), ValueError),
                        (dict(table=z(4, 9, 2).cpu()), Exception), (dict(row_of_element=z(4, dt=torch.int64)), TypeError),
                        (dict(row_of_element=z(3, dt=torch.int32)), ValueError),
                        (dict(row_of_element=torch.tensor([0, 1, 2, 4], dtype=torch.int32, device=dev)), ValueError),
                        (dict(row_of_element=torch.tensor([0, -2, 2, 3], dtype=torch.int32, device=dev)), ValueError)):
        b = mk()
        for k, v in change.items():
            setattr(b, k, v)
        with pytest.raises(err):
            ops.facet_source_terms(y, b, None, stage=np.zeros(6))


# ---- 9. the point kernel ---------------------------------------------------------------------------------------------------------------
def _kernel_points(mesh, m, rng):
    """m points of a 3 x 3 x 3 box (as tests/test_point_sources_gpu.py): two coincident, several in one cell, one on a cell vertex
    (one-hot weights), one on a face shared by two cells; the rest anywhere inside."""
    L, h = mesh.length[0], mesh.h[0]
    if m == 0:
        return np.zeros((0, 3))
    if m == 1:
        return np.array([[0.41 * L, 0.57 * L, 0.23 * L]])
    special = np.array([[0.3 * h, 1.4 * h, 2.2 * h], [0.3 * h, 1.4 * h, 2.2 * h], [1.2 * h, 1.3 * h, 1.1 * h], [1.7 * h, 1.6 * h, 1.5 * h],
                        [1.5 * h, 1.1 * h, 1.9 * h], [h, 2 * h, h], [2 * h, 0.4 * h, 0.6 * h]])
    rest = rng.uniform(0.02 * L, 0.98 * L, (m - special.shape[0], 3))
    rest[:, 0] *= 0.65  # x < 2 h: the interiors of the last layer of cells hold no point
    return np.concatenate([special, rest])


@pytest.mark.parametrize("m", [0, 1, 300])
@pytest.mark.parametrize("P", DEGREES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_point_wave_kernel(dtype, P, m):
    """y += the points' terms on a y filled with non-zero values, against np.add.at in fp64: 5 rows for 300 points, every ninth point
    silent (row -1), the delays cycling through the time cases of the facet test; the vertex point (one-hot rows) fires.  Entries no
    active point's cell holds keep their bits, and with every point outside the table all of y does."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, src, sensors, ops = pkg("boxmesh"), pkg("sources"), pkg("sensors"), pkg("operators")
    mesh = boxmesh.BoxMesh(P, (3, 3, 3), length=0.003)
    rng = np.random.default_rng(1000 * P + m)
    pts = _kernel_points(mesh, m, rng)
    nt, R = 33, 5
    wf = _random_table(rng, R, nt)
    delay = _delays(nt, m + 2)[2:]  # (m == 1: inside an interval)
    row_of = np.where(np.arange(m) % 9 == 8, -1, np.arange(m) % R)
    if m == 300:
        delay[5], row_of[5] = _delays(nt, 4)[3], 2  # the vertex point: exactly on an interior node
    ps = src.PointSources(pts, amplitude=rng.uniform(0.5, 2.0, m), delay=delay, waveform=wf, waveform_of_point=row_of)
    su = sensors.sensor_setup(mesh, pts)
    assert su.point_ids.size == m
    if m == 300:
        vertex = su.weights[np.nonzero(su.point_ids == 5)[0][0]]
        assert np.all(np.sort(np.abs(vertex), axis=1)[:, :-1] < 1e-12) and np.allclose(np.abs(vertex).max(axis=1), 1.0)
    y0 = (rng.uniform(0.5, 2.0, mesh.ndofs) * rng.choice([-1.0, 1.0], mesh.ndofs)).astype(dtype)
    g, _ = ps.values(T_STAGE, F0)
    if m == 300:
        x = (T_STAGE - delay - T0_TAB) / DT_TAB
        assert np.array_equal(g != 0.0, (x >= 0) & (x <= nt - 1) & (row_of >= 0)) and g[5] == ps.amplitude[5] * wf.samples[2, 11]
        assert all(np.any(np.isclose(x, c)) for c in _time_cases(nt))
    active = g[su.point_ids] != 0.0
    ref = point_source_cpu.inject(y0.astype(np.float64), su, g[su.point_ids], P + 1)
    bound = ps.bind(mesh, dtype, torch.device("cuda", 0), F0, setup=su)
    assert bound.npoints == m and (m == 0 or bound.table.shape[1:] == (nt, 2))
    y = torch.from_numpy(y0).cuda()
    ops.point_source_terms(y, bound, bound.stage_scalars(T_STAGE))
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    tol = TOL[np.dtype(dtype)]
    assert rel_l2(got, ref) < tol["l2"] and rel_max(got, ref) < tol["mx"]
    touched = np.zeros(mesh.ndofs, dtype=bool)
    touched[su.rows[su.cell_index[active]].reshape(-1)] = True
    assert np.array_equal(got[~touched].view(np.uint8), y0[~touched].view(np.uint8))
    if m:
        assert touched.any() and not touched.all() and np.any(got[touched] != y0[touched])
        idle = src.PointSources(pts, delay=np.where(np.arange(m) % 2 == 0, _delays(nt, 1)[0], _delays(nt, 6)[5]), waveform=wf,
                                waveform_of_point=np.arange(m) % R)
        assert not np.any(idle.values(T_STAGE, F0)[0])
        b2 = idle.bind(mesh, dtype, torch.device("cuda", 0), F0, setup=su)
        y = torch.from_numpy(y0).cuda()
        ops.point_source_terms(y, b2, b2.stage_scalars(T_STAGE))
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy().view(np.uint8), y0.view(np.uint8))


# ---- 10. the solvers: a sampled analytic source is the analytic source -------------------------------------------------------------------
def _array3(L, **kw):
    src = pkg("sources")
    return src.SourceArray(src.grid_elements(3, 1, (0.0, L), (0.0, L)), n_elements=3, **kw)


@pytest.mark.parametrize("form", ["linear-fused-lean", "linear-reference-sequence", "westervelt-fused"])
def test_sampled_analytic_array_equals_analytic_array(form):
    """A 3-element array with distinct amplitudes, phases and delays (multiples of half a step), driven analytically and by the table
    of its waveform sampled at half the step with the analytic derivative (R = E, the phases folded into the rows): every stage time
    is a node of the table, and u and v after 30 steps agree to 1e-11."""
    import torch

    torch.cuda.set_device(0)
    boxmesh = pkg("boxmesh")
    P, L, K = 3, 0.006, 30
    mesh = boxmesh.BoxMesh(P, (3, 3, 3), length=L, perturb=0.1, seed=3)
    if form.startswith("linear"):
        f0 = F0
        mk = lambda a: pkg("linear_solver").LinearSpectral3D(mesh, np.float64, fused=form == "linear-fused-lean", source=a)  # noqa: E731
    else:
        f0 = 1.1e6
        mk = lambda a: pkg("nonlinear_solver").WesterveltSpectral3D(mesh, np.float64, fused=True, source=a)  # noqa: E731
    dt, _, _ = _dt(mesh, P, L, 1500.0 if form.startswith("linear") else 1480.0, f0)
    amp, phase, delay = np.array([1.0, 0.4, 1.3]), np.array([0.0, 0.9, -2.0]), np.array([0.0, 3.0, 8.0]) * 0.5 * dt
    ana = _array3(L, amplitude=amp, phase=phase, delay=delay)
    wf = waveform_cpu.analytic_table(ana, f0, 0.5 * dt, 2 * K + 2)
    out = []
    for a in (ana, _array3(L, amplitude=amp, delay=delay, waveform=wf)):
        s = mk(a)
        if form == "linear-fused-lean":
            assert s.lean_stages
        s.init()
        _, steps = s.rk4(0.0, 1.0, dt, max_steps=K)
        assert steps == K and (s.source.table is None) == (a is ana)
        out.append((s.u_sol(), s.v_sol()))
    (u0, v0), (u1, v1) = out
    print(f"{form}: u rel l2 {rel_l2(u1, u0):.3e} max {rel_max(u1, u0):.3e}, v rel l2 {rel_l2(v1, v0):.3e} max {rel_max(v1, v0):.3e}")
    assert np.max(np.abs(u0)) > 0 and np.max(np.abs(v0)) > 0
    assert rel_l2(u1, u0) <= 1e-11 and rel_l2(v1, v0) <= 1e-11 and rel_max(u1, u0) <= 1e-11 and rel_max(v1, v0) <= 1e-11


# ---- 11. the solvers against the CPU model ------------------------------------------------------------------------------------------------
_model_cache = {}


def _bowl_warp(xg):
    L = 0.006
    y, z = xg[:, 1] / L - 0.5, xg[:, 2] / L - 0.5
    out = xg.copy()
    out[:, 0] = xg[:, 0] + 0.15 * L * (y * y + z * z) * (1.0 - xg[:, 0] / L)
    return out


def _pulse_case(solver, kind, oracle_c):
    """Mesh, step, the source driven by Gaussian pulses (one row per element / point, sampled at a third of the step: the stage times
    fall INSIDE the intervals) and the CPU model's (u, v), computed once."""
    key = (solver, kind)
    if key not in _model_cache:
        boxmesh, src = pkg("boxmesh"), pkg("sources")
        P, L, K = 3, 0.006, 12
        lin = solver == "linear"
        f0, c0 = (F0, 1500.0) if lin else (1.1e6, 1480.0)
        mesh = boxmesh.BoxMesh(P, (4, 3, 3), length=L, perturb=0.1, seed=2) if lin else boxmesh.BoxMesh(P, (4, 3, 3), length=L, warp=_bowl_warp)
        dt, tf, _ = _dt(mesh, P, L, c0, f0)
        wf = waveform_cpu.pulse_waveform(f0, dt / 3.0, 3 * K + 2, t_c=5.0 * dt, cycles=2.5 * dt * f0, rows=3)
        if kind == "array":
            source = _array3(L, amplitude=[1.0, 0.4, 1.3], delay=np.array([0.0, 1.7, 0.6]) * dt, waveform=wf)
            A = P0 * 2 * np.pi * f0 / c0 if lin else 2.0 * (1000.0 * c0 * 0.38557513826589934) * 2 * np.pi * f0 / c0
            term = waveform_cpu.array_term(mesh, source, f0, A)
        else:
            pts = np.array([[0.41, 0.57, 0.36], [0.68, 0.31, 0.62], [0.22, 0.45, 0.71]]) * L
            source = src.PointSources(pts, amplitude=[0.05, 0.03, 0.04], delay=np.array([0.0, 2.5, 0.4]) * dt, waveform=wf,
                                      waveform_of_point=[0, 2, -1])
            A = None
            term = point_source_cpu.point_term(mesh, source, f0)
        solve = rk4_oracle.solve if lin else rk4_oracle.solve_westervelt
        ref = solve(mesh, K, dt, source_term=term, oracle_c=oracle_c)
        for a in ref:
            a.setflags(write=False)
        _model_cache[key] = (mesh, dt, tf, K, source, A, ref)
    return _model_cache[key]


@pytest.mark.parametrize("kind", ["array", "points"])
@pytest.mark.parametrize("solver", ["linear", "westervelt"])
def test_solver_with_a_pulse_matches_model(oracle_c, solver, kind):
    """12 steps driven by Gaussian pulses of 2.5 steps' width from a table: the fused solvers against ``oracle.rk4_oracle`` with a
    ``source_term`` hook that calls ``SourceArray.values`` / ``PointSources.values``, to 1e-11."""
    import torch

    torch.cuda.set_device(0)
    mesh, dt, tf, K, source, A, (u_ref, v_ref) = _pulse_case(solver, kind, oracle_c)
    cls = pkg("linear_solver").LinearSpectral3D if solver == "linear" else pkg("nonlinear_solver").WesterveltSpectral3D
    kw = dict(source=source) if kind == "array" else dict(source_amplitude=0.0, point_source=source)
    s = cls(mesh, np.float64, fused=True, **kw)
    if kind == "array":
        assert abs(s.source.scale - A) <= 1e-15 * A and s.source.table is not None
    else:
        assert s._points.npoints == 3 and tuple(s._points.table.shape[:1]) == (2,) and s._points.row_of_point.cpu().tolist().count(-1) == 1
    s.init()
    _, steps = s.rk4(0.0, tf, dt, max_steps=K)
    assert steps == K
    du, dv = rel_l2(s.u_sol(), u_ref[: mesh.nlocal]), rel_l2(s.v_sol(), v_ref[: mesh.nlocal])
    print(f"{solver} {kind}: rel l2 to the model u {du:.3e} v {dv:.3e}; max |u_ref| {np.max(np.abs(u_ref)):.3e}")
    assert np.max(np.abs(u_ref)) > 0 and np.max(np.abs(v_ref)) > 0
    assert du < 1e-11 and dv < 1e-11


# ---- 12. hipGraph replay and partitioned runs -----------------------------------------------------------------------------------------------
def _pulse_array4(L, dt, f0=F0, nt=64):
    src = pkg("sources")
    wf = waveform_cpu.pulse_waveform(f0, dt / 3.0, nt, t_c=5.0 * dt, cycles=2.5 * dt * f0, rows=4)
    return src.SourceArray(src.grid_elements(2, 2, (0.0, L), (0.0, L)), n_elements=4, amplitude=[1.0, 0.5, 0.8, 1.2],
                           delay=np.array([0.0, 0.3, 0.9, 0.6]) * dt, waveform=wf)


@pytest.mark.parametrize("solver", ["linear", "westervelt"])
def test_graph_replay_with_a_waveform_array_equals_rk4(solver):
    """The stage block of a captured step is the six words it was: the replayed graph reads t and A of every stage from the slot."""
    import torch

    torch.cuda.set_device(0)
    boxmesh = pkg("boxmesh")
    P, L, K = 3, 0.006, 12
    mesh = boxmesh.BoxMesh(P, (4, 3, 3), length=L, perturb=0.1, seed=3)
    f0, c0 = (F0, 1500.0) if solver == "linear" else (1.1e6, 1480.0)
    dt, tf, _ = _dt(mesh, P, L, c0, f0)
    cls = pkg("linear_solver").LinearSpectral3D if solver == "linear" else pkg("nonlinear_solver").WesterveltSpectral3D
    out = []
    for graph in (False, True):
        s = cls(mesh, np.float64, fused=True, source=_pulse_array4(L, dt, f0))
        s.init()
        _, steps = (s.rk4_graph if graph else s.rk4)(0.0, tf, dt, max_steps=K)
        assert steps == K
        out.append((s.u_sol(), s.v_sol()))
    assert np.max(np.abs(out[0][0])) > 0
    assert rel_max(out[1][0], out[0][0]) <= 1e-12 and rel_max(out[1][1], out[0][1]) <= 1e-12


def test_graph_replay_with_waveform_points_is_refused():
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, lib_mod, src = pkg("boxmesh"), pkg("linear_solver"), pkg("_lib"), pkg("sources")
    mesh = boxmesh.BoxMesh(2, (3, 3, 3), length=0.006)
    ps = src.PointSources([[0.002, 0.003, 0.0025]], waveform=waveform_cpu.pulse_waveform(F0, 1e-8, 40, 1e-7, 0.05))
    s = ls.LinearSpectral3D(mesh, np.float64, point_source=ps)
    s.init()
    with pytest.raises(lib_mod.FusGpuError, match="point_source"):
        s.rk4_graph(0.0, 1e-6, 1e-7, max_steps=2)
    assert not hasattr(s, "_graphs") and not np.any(s.u_sol())


def test_partitioned_waveform_array_equals_single_rank():
    """Two ranks sharing cuda:0 in this process (in-process transport), each binding its own source facets by centroid and uploading
    the two table rows they use: the owned dofs equal the single-rank run."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, scat, utils = pkg("boxmesh"), pkg("linear_solver"), pkg("scatterer"), pkg("utils")
    P, cells, L, K, grid, R = 3, (4, 4, 4), 0.006, 10, (1, 2, 1), 2
    serial = boxmesh.BoxMesh(P, cells, length=L)
    dt, _, _ = _dt(serial, P, L)
    one = ls.LinearSpectral3D(serial, np.float64, source=_pulse_array4(L, dt))
    one.init()
    one.rk4(0.0, 1.0, dt, max_steps=K)
    ref = np.empty(serial.ndofs_global)
    ref[serial.global_lexicographic_ids()[: serial.nlocal]] = one.u_sol()
    meshes = [boxmesh.BoxMesh(P, cells, grid=grid, rank=r, length=L, ghost_order=5) for r in range(R)]
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    solvers = [ls.LinearSpectral3D(meshes[r], np.float64, comm=scat.NativeComm(local=(8530, R, r)), halo_plan=(od[r], gd[r]),
                                   defer_setup_exchange=True, source=_pulse_array4(L, dt)) for r in range(R)]
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        s.init()
    res = _lockstep([s.rk4_schedule(0.0, 1.0, dt, K) for s in solvers])
    torch.cuda.synchronize()
    for s in solvers:
        s.check_halo_health("test")
    assert all(r[1] == K for r in res) and tuple(one.source.table.shape[:1]) == (4,)
    # each rank holds two of the four elements: two rows uploaded, the other elements' rows -1
    assert [tuple(s.source.table.shape[:1]) for s in solvers] == [(2,), (2,)]
    assert sorted(s.source.row_of_element.cpu().tolist().count(-1) for s in solvers) == [2, 2]
    assert np.max(np.abs(ref)) > 0
    for m, s in zip(meshes, solvers):
        mine = ref[m.global_lexicographic_ids()[: m.nlocal]]
        assert np.max(np.abs(s.u_sol() - mine)) <= 1e-11 * np.max(np.abs(ref))


# ---- 13. time reversal of the signals, end to end ---------------------------------------------------------------------------------------
def test_time_reversed_signals_refocus_through_the_slab():
    """The slab case of tests/test_receivers_gpu.py (waveform_cpu.slab_case: same mesh, medium and array; the slab keeps its thickness
    of two cells, one water wavelength) with a pulse.  Listen run: a point source at the focus emits
    exp(-((t - 4T) / T)^2 / 2) cos(w0 (t - 4T)) from a table and the nine elements record all 798 steps (T_run = 14 T).  Transmit run:
    ``time_reversed_waveform`` fires the array and a point sensor records at the focus.

    Derivable condition: element e hears the pulse centre at t_c + tau_e and re-emits it at T_run - t_c - tau_e, so every path brings
    it back to the focus at T_run - t_c = 10 T; the drive and the pressure differ by a quarter period of carrier phase, the envelope
    peak does not move: the largest |p| lies within half a period of 10 T.  Amplitude condition: that peak against the peak of the
    same pulse fired with ``focus_delays`` computed in water, at least half the ratio of the CPU model.  The CPU model
    (``python tests/waveform_cpu.py``: oracle/rk4_oracle operators, 3 x 798 steps) gives 2.403195e+05 Pa at 10.0000 T for the
    time-reversed signals and 5.708349e+04 Pa at 9.3158 T for the geometric delays: ratio 4.21, so at least 2.105 here."""
    import torch

    torch.cuda.set_device(0)
    ls, src, rx_mod, sensors = pkg("linear_solver"), pkg("sources"), pkg("receivers"), pkg("sensors")
    case = waveform_cpu.slab_case()
    mesh, dt, nsteps, focus, fn = case["mesh"], case["dt"], case["nsteps"], case["focus"], case["fn"]
    assert nsteps == 798 and 0 < np.count_nonzero(case["c"] == 3000.0) == 2 * 3 * 6
    kw = dict(speed_of_sound=case["c"], density=case["rho"], reference_speed_of_sound=1500.0)
    listen = ls.LinearSpectral3D(mesh, np.float64, source_amplitude=0.0, point_source=src.PointSources(focus, waveform=case["pulse"]), **kw)
    rx = rx_mod.ElementReceivers(mesh, fn, np.float64, capacity=nsteps, n_elements=9, detJ=listen.detJ_f1)
    listen.init()
    _, steps = listen.rk4(0.0, 1.0, dt, max_steps=nsteps, receivers=rx)
    assert steps == nsteps and rx.nrec == nsteps and np.all(np.abs(rx.series()).max(axis=0) > 0)

    def transmit(array):
        s = ls.LinearSpectral3D(mesh, np.float64, source=array, **kw)
        probe = sensors.PointSensors(mesh, focus, np.float64, capacity=nsteps)
        s.init()
        s.rk4(0.0, 1.0, dt, max_steps=nsteps, sensors=probe)
        p = np.abs(probe.series()[:, 0])
        k = int(np.argmax(p))
        return float(p[k]), (k + 1) * dt

    arr = rx_mod.time_reversed_waveform(rx, dt)
    assert arr.waveform.n_samples == nsteps and arr.waveform_of_element.tolist() == list(range(9))
    p_tr, t_tr = transmit(arr)
    p_geo, t_geo = transmit(src.SourceArray(fn, delay=src.focus_delays(case["centres"], focus[0], 1500.0), n_elements=9,
                                            waveform=case["pulse"]))
    t_focus = nsteps * dt - case["t_c"]
    print(f"{nsteps} steps; peak |p| at the focus: time-reversed signals {p_tr:.6e} at {t_tr / T0:.4f} T (T_run - t_c = {t_focus / T0:.4f} T), "
          f"geometric delays {p_geo:.6e} at {t_geo / T0:.4f} T; ratio {p_tr / p_geo:.4f}")
    assert abs(t_tr - t_focus) <= 0.5 * T0
    assert p_tr / p_geo >= 0.5 * 4.21


# ---- 14. the demo ---------------------------------------------------------------------------------------------------------------------------
def test_linear_box_demo_pulse_time_reversal_reports_the_refocus_time():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fenicsx-fus-gpu_amd", "demo_linear_box.py"), "--length", "0.012", "--cells", "8",
                        "--time-reversal", "0.011", "0.0063", "0.0058", "--elements", "3", "3", "--pulse", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {ln.split(":")[0]: ln.split(":", 1)[1] for ln in r.stdout.splitlines() if ln.startswith(("Refocus", "Peak"))}
    assert "Refocus time" in got and float(got["Refocus time"].split(" s")[0]) > 0.0, r.stdout
    off = float(got["Refocus time"].split(", ")[1].split(" periods")[0])
    assert off <= 0.5, r.stdout  # within half a period of T_run - t_c
    assert float(got["Peak |p| at the focus"].split("ratio ")[1]) > 0.0


def test_linear_box_demo_source_waveform(tmp_path):
    """--source-waveform with one row drives the whole face; with --array and one row per element, the elements."""
    t = np.arange(400) * 2.5e-8
    np.save(tmp_path / "one.npy", waveform_cpu.gaussian_pulse(t, F0, 2 * T0)[0])
    np.save(tmp_path / "six.npy", np.stack([waveform_cpu.gaussian_pulse(t, F0, (2 + 0.1 * e) * T0)[0] for e in range(6)]))
    demo = os.path.join(ROOT, "fenicsx-fus-gpu_amd", "demo_linear_box.py")
    for extra, rows in ((["--source-waveform", str(tmp_path / "one.npy"), "2.5e-8"], 1),
                        (["--array", "2,3", "--source-waveform", str(tmp_path / "six.npy"), "2.5e-8"], 6)):
        r = subprocess.run([sys.executable, demo, "--cells", "6", "--degree", "2", "--max-steps", "30"] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0 and "Solve time per step" in r.stdout, r.stdout + r.stderr
        assert f"Source waveform: {rows} row(s) of 400 samples" in r.stdout
    r = subprocess.run([sys.executable, demo, "--cells", "6", "--degree", "2", "--array", "2,2", "--source-waveform", str(tmp_path / "six.npy"),
                        "2.5e-8"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--source-waveform" in r.stderr  # six rows for four elements
