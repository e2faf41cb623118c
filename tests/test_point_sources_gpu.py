"""Point sources on the GPU: the kernel (csrc/point_source.hpp) against numpy and as the adjoint of the probe, both wave solvers with
point sources -- every stage implementation -- against the CPU model (oracle/rk4_oracle.py with the source hook of
tests/point_source_cpu.py), ``None`` and the empty set, hipGraph replay (refused) and fp32."""

import numpy as np
import pytest

import point_source_cpu
from conftest import TOL, pkg, rel_l2, rel_max
from oracle import rk4_oracle

pytestmark = pytest.mark.gpu

F0 = 0.5e6
T0 = 1.0 / F0
# every degree point_source_kernel is compiled for (tests/test_cell_model64.py compares this list with the compiled names)
DEGREES = list(range(1, 11))


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
def _kernel_points(mesh, m, rng):
    """m points of a 3 x 3 x 3 box: two coincident, several in one cell, one on a cell vertex (one-hot weights), one on a face shared
    by two cells; the rest anywhere inside."""
    L, h = mesh.length[0], mesh.h[0]
    if m == 0:
        return np.zeros((0, 3))
    if m == 1:
        return np.array([[0.41 * L, 0.57 * L, 0.23 * L]])
    special = np.array([[0.3 * h, 1.4 * h, 2.2 * h], [0.3 * h, 1.4 * h, 2.2 * h],  # coincident
                        [1.2 * h, 1.3 * h, 1.1 * h], [1.7 * h, 1.6 * h, 1.5 * h], [1.5 * h, 1.1 * h, 1.9 * h],  # one cell
                        [h, 2 * h, h],  # a vertex shared by eight cells
                        [2 * h, 0.4 * h, 0.6 * h]])  # a face shared by two cells
    rest = rng.uniform(0.02 * L, 0.98 * L, (m - special.shape[0], 3))
    rest[:, 0] *= 0.65  # x < 2 h: the interiors of the last layer of cells hold no point, so some of y is touched by none
    return np.concatenate([special, rest])


@pytest.mark.parametrize("m", [0, 1, 300])
@pytest.mark.parametrize("P", DEGREES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_point_source_kernel(dtype, P, m):
    """y += the points' terms at t = 12.3 T of a burst of 12 T, on a y filled with non-zero values, against np.add.at in fp64.  The
    delays put a quarter of the points before their start, on the ramp, on the plateau and after the burst; entries no active point's
    cell holds keep their bits, and with every point outside its burst all of y does."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, src, sensors, ops = pkg("boxmesh"), pkg("sources"), pkg("sensors"), pkg("operators")
    mesh = boxmesh.BoxMesh(P, (3, 3, 3), length=0.003)
    rng = np.random.default_rng(1000 * P + m)
    pts = _kernel_points(mesh, m, rng)
    t, D = 12.3 * T0, 12 * T0
    delays = np.array([13 * T0, 11 * T0, 5 * T0, 0.0])  # s = t - delay: < 0, on the ramp up, on the plateau, > D
    delay = delays[(np.arange(m) + 2) % 4] if m else np.zeros(0)  # (m == 1: the plateau)
    if m == 300:
        delay[:2] = 5 * T0  # the coincident pair both fire
        delay[5:7] = [11 * T0, 5 * T0]  # ... and the vertex and the face point
    ps = src.PointSources(pts, amplitude=rng.uniform(0.5, 2.0, m), phase=rng.uniform(-3.0, 3.0, m), delay=delay, duration=D)
    su = sensors.sensor_setup(mesh, pts)
    assert su.point_ids.size == m
    if m == 300:
        vertex = su.weights[np.nonzero(su.point_ids == 5)[0][0]]
        assert np.all(np.sort(np.abs(vertex), axis=1)[:, :-1] < 1e-12) and np.allclose(np.abs(vertex).max(axis=1), 1.0)  # one-hot rows
    y0 = (rng.uniform(0.5, 2.0, mesh.ndofs) * rng.choice([-1.0, 1.0], mesh.ndofs)).astype(dtype)
    g, _ = ps.values(t, F0)
    active = g[su.point_ids] != 0.0
    if m:
        s = t - delay
        assert {bool(x) for x in (s < 0)} == {True, False} or m == 1
        assert np.array_equal(g != 0.0, (s > 0) & (s < D))
        assert m == 1 or (np.any((s > 0) & (s < 4 * T0)) and np.any((s > 4 * T0) & (s < D - 4 * T0)) and np.any(s > D))
    ref = point_source_cpu.inject(y0.astype(np.float64), su, g[su.point_ids], P + 1)
    bound = ps.bind(mesh, dtype, torch.device("cuda", 0), F0, setup=su)
    assert bound.npoints == m
    y = torch.from_numpy(y0).cuda()
    ops.point_source_terms(y, bound, bound.stage_scalars(t))
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    tol = TOL[np.dtype(dtype)]
    assert rel_l2(got, ref) < tol["l2"] and rel_max(got, ref) < tol["mx"]
    touched = np.zeros(mesh.ndofs, dtype=bool)
    touched[su.rows[su.cell_index[active]].reshape(-1)] = True
    assert np.array_equal(got[~touched].view(np.uint8), y0[~touched].view(np.uint8))
    if m:
        assert touched.any() and not touched.all() and np.any(got[touched] != y0[touched])
        # every point outside its burst: no atomic is issued, all of y keeps its bits
        idle = src.PointSources(pts, delay=np.where(np.arange(m) % 2 == 0, 13 * T0, 0.0), duration=D)
        assert not np.any(idle.values(t, F0)[0])
        b2 = idle.bind(mesh, dtype, torch.device("cuda", 0), F0, setup=su)
        y = torch.from_numpy(y0).cuda()
        ops.point_source_terms(y, b2, b2.stage_scalars(t))
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy().view(np.uint8), y0.view(np.uint8))


@pytest.mark.parametrize("P", DEGREES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_point_source_is_the_adjoint_of_the_probe(dtype, P):
    """With ONE SensorSetup: sum_j inject(q)[j] x[j] == sum_p q_p probe(x)_p for random x and q, relative to the sum of the terms'
    magnitudes.  At t = 8 T (delay 0, phase 0) the waveform is exactly 1 -- the plateau, cospi(16) -- so the monopole strength is q."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, src, sensors, ops = pkg("boxmesh"), pkg("sources"), pkg("sensors"), pkg("operators")
    mesh = boxmesh.BoxMesh(P, (3, 3, 3), length=0.003, perturb=0.1, seed=7)
    rng = np.random.default_rng(P)
    m = 200
    pts = rng.uniform(0.0004, 0.0026, (m, 3))
    q = rng.standard_normal(m)
    x = rng.standard_normal(mesh.ndofs).astype(dtype)
    probe = sensors.PointSensors(mesh, pts, dtype)
    assert probe.m == m
    x_d = torch.from_numpy(x).cuda()
    px = probe.evaluate(x_d).cpu().numpy().astype(np.float64)  # columns of probe.point_ids
    ps = src.PointSources(pts, amplitude=q)
    assert np.array_equal(ps.values(8 * T0, F0)[0], q)
    bound = ps.bind(mesh, dtype, torch.device("cuda", 0), F0, setup=probe.setup)
    assert np.array_equal(bound.point_ids, probe.point_ids)
    y = torch.zeros(mesh.ndofs, dtype=x_d.dtype, device="cuda")
    ops.point_source_terms(y, bound, bound.stage_scalars(8 * T0))
    torch.cuda.synchronize()
    yx = y.cpu().numpy().astype(np.float64) * x.astype(np.float64)
    qp = q[probe.point_ids] * px
    scale = np.abs(yx).sum() + np.abs(qp).sum()
    print(f"P {P} {np.dtype(dtype).name}: <inject(q), x> {yx.sum():.15e}  <q, probe(x)> {qp.sum():.15e}  sum |terms| {scale:.3e}")
    assert scale > 0 and abs(yx.sum() - qp.sum()) < TOL[np.dtype(dtype)]["l2"] * scale


def test_point_source_terms_argument_checks():
    import torch

    torch.cuda.set_device(0)
    boxmesh, src, ops, lib_mod = pkg("boxmesh"), pkg("sources"), pkg("operators"), pkg("_lib")
    mesh = boxmesh.BoxMesh(2, (2, 2, 2), length=0.002)
    dev = torch.device("cuda", 0)
    ps = src.PointSources([[0.0005, 0.0007, 0.0011], [0.0015, 0.0003, 0.0009]])
    b = ps.bind(mesh, np.float64, dev, F0)
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(TypeError):
        ops.point_source_terms(z(mesh.ndofs, torch.float32), b, b.stage_scalars(0.0))
    with pytest.raises(ValueError):
        ops.point_source_terms(z(mesh.ndofs - 1), b, b.stage_scalars(0.0))
    with pytest.raises(ValueError):
        ops.point_source_terms(z(mesh.ndofs), b, [0.0, 1.0])
    with pytest.raises(lib_mod.FusGpuError):
        ops.point_source_terms(z(mesh.ndofs).cpu(), b, b.stage_scalars(0.0))  # no CPU path
    with pytest.raises(ValueError, match="outside"):
        src.PointSources([[0.0005, 0.0007, 0.0011], [0.5, 0.0, 0.0]]).bind(mesh, np.float64, dev, F0)


# ---- the solvers against the CPU model -----------------------------------------------------------------------------------------------
_LINEAR = {"box": dict(P=4, cells=(6, 3, 3), length=(0.012, 0.006, 0.006), mesh_kw={}, solver_kw={}, steps=12),
           "perturbed-in-kernel-geometry": dict(P=3, cells=(5, 4, 4), length=0.01, mesh_kw=dict(perturb=0.1, seed=2),
                                                solver_kw=dict(in_kernel_geometry=True), steps=12)}
_model_cache = {}


def _two_points(mesh, dt):
    """Two interior points with different amplitude, phase and delay (both fire within the run)."""
    L = np.asarray(mesh.length)
    return pkg("sources").PointSources(np.array([[0.41, 0.57, 0.36], [0.68, 0.31, 0.62]]) * L, amplitude=[0.05, 0.03], phase=[0.0, 1.1],
                                       delay=[0.0, 2.5 * dt])


def _linear_case(name, oracle_c):
    """Mesh, time step, the points and -- computed once per case -- the model's fields: the points alone (no facet source), the
    points with the scalar facet source, and the facet source alone."""
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    if name not in _model_cache:
        k = _LINEAR[name]
        mesh = boxmesh.BoxMesh(k["P"], k["cells"], length=k["length"], **k["mesh_kw"])
        h = ls.time_step_parameters(mesh, k["P"], 1500.0, F0, mesh.length[0])
        dt, tf, _ = ls.snap_time_step(h, k["P"], 1500.0, F0, mesh.length[0])
        ps = _two_points(mesh, dt)
        alone = rk4_oracle.solve(mesh, k["steps"], dt, source_term=point_source_cpu.point_term(mesh, ps, F0), oracle_c=oracle_c)
        both = rk4_oracle.solve(mesh, k["steps"], dt, oracle_c=oracle_c,
                                source_term=point_source_cpu.point_term(mesh, ps, F0, facet_scale=(60000.0 * 2 * np.pi * F0 / 1500.0, 4.0)))
        facet = rk4_oracle.solve(mesh, k["steps"], dt, oracle_c=oracle_c)
        for a in alone + both + facet:
            a.setflags(write=False)
        _model_cache[name] = (mesh, dt, tf, ps, alone, both, facet)
    return _model_cache[name]


@pytest.mark.parametrize("variant", ["fused-lean", "fused-reference-kinds", "reference-sequence"])
@pytest.mark.parametrize("case", list(_LINEAR) + ["box-with-facet-source"])
def test_linear_solver_with_points_matches_model(oracle_c, case, variant):
    """Two interior points, 12 steps, the facet source silenced (``source_amplitude=0.0``) -- and, on the box, once with the scalar
    facet source active too: the fused stage with the lean vector pass, with the reference's stage kinds and the reference launch
    sequence, each against the CPU model at the bar of tests/test_solver_gpu.py; and the points are not a no-op."""
    import torch

    torch.cuda.set_device(0)
    ls = pkg("linear_solver")
    name = case.replace("-with-facet-source", "")
    with_facets = name != case
    mesh, dt, tf, ps, alone, both, facet = _linear_case(name, oracle_c)
    (u_ref, v_ref), (u_free, v_free) = (both, facet) if with_facets else (alone, (np.zeros_like(alone[0]),) * 2)
    k = _LINEAR[name]
    s = ls.LinearSpectral3D(mesh, np.float64, fused=variant != "reference-sequence", point_source=ps,
                            **({} if with_facets else dict(source_amplitude=0.0)), **k["solver_kw"])
    if k["solver_kw"]:
        assert s.in_kernel_geometry
    if variant == "fused-reference-kinds":
        s.lean_stages = False
    assert s._points.npoints == 2
    s.init()
    _, steps = s.rk4(0.0, tf, dt, max_steps=k["steps"])
    assert steps == k["steps"]
    u, v = s.u_sol(), s.v_sol()
    du, dv = rel_l2(u, u_ref), rel_l2(v, v_ref)
    far = np.linalg.norm(u - u_free) / np.linalg.norm(u_ref)
    print(f"{case} {variant}: rel l2 to the model u {du:.3e} v {dv:.3e}; distance to the point-free model / |u| {far:.3e}")
    assert np.max(np.abs(u_ref)) > 0
    assert du < 1e-11 and dv < 1e-11
    assert far > 1e-3 and np.linalg.norm(v - v_free) / np.linalg.norm(v_ref) > 1e-3


def _bowl_warp(xg):
    """Smooth non-affine map: the x = 0 face bulges like a bowl (as tests/test_solver_gpu.py)."""
    L = 0.006
    y, z = xg[:, 1] / L - 0.5, xg[:, 2] / L - 0.5
    out = xg.copy()
    out[:, 0] = xg[:, 0] + 0.15 * L * (y * y + z * z) * (1.0 - xg[:, 0] / L)
    return out


def _westervelt_case(oracle_c):
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    if "westervelt" not in _model_cache:
        P, L, steps = 4, 0.006, 10
        mesh = boxmesh.BoxMesh(P, (4, 3, 3), length=L, warp=_bowl_warp)
        h = ls.time_step_parameters(mesh, P, 1480.0, 1.1e6, L)
        dt, tf, _ = ls.snap_time_step(h, P, 1480.0, 1.1e6, L)
        ps = _two_points(mesh, dt)
        ref = rk4_oracle.solve_westervelt(mesh, steps, dt, source_term=point_source_cpu.point_term(mesh, ps, 1.1e6), oracle_c=oracle_c)
        for a in ref:
            a.setflags(write=False)
        _model_cache["westervelt"] = (mesh, dt, tf, steps, ps, ref)
    return _model_cache["westervelt"]


@pytest.mark.parametrize("variant", ["fused-two-gather", "fused-uniform-ratio", "reference-sequence"])
def test_westervelt_solver_with_points_matches_model(oracle_c, variant):
    """Bowl-warped cells, 10 steps, two interior points and no facet source: the fused stage with the two-gather and the single-gather
    cell pass and the reference launch sequence, each against the CPU model."""
    import torch

    torch.cuda.set_device(0)
    nls = pkg("nonlinear_solver")
    mesh, dt, tf, steps, ps, (u_ref, v_ref) = _westervelt_case(oracle_c)
    s = nls.WesterveltSpectral3D(mesh, np.float64, fused=variant != "reference-sequence", uniform_ratio=variant == "fused-uniform-ratio",
                                 source_amplitude=0.0, point_source=ps)
    assert (s.kappa is not None) == (variant == "fused-uniform-ratio") and s.p0 == 0.0
    s.init()
    _, done = s.rk4(0.0, tf, dt, max_steps=steps)
    assert done == steps
    u, v = s.u_sol(), s.v_sol()
    du, dv = rel_l2(u, u_ref), rel_l2(v, v_ref)
    print(f"westervelt {variant}: rel l2 to the model u {du:.3e} v {dv:.3e}; max |u_ref| {np.max(np.abs(u_ref)):.3e}")
    assert np.max(np.abs(u_ref)) > 0
    assert du < 1e-11 and dv < 1e-11
    assert np.linalg.norm(u) / np.linalg.norm(u_ref) > 1e-3  # the point-free run with a silenced facet source is zero


# ---- None and the empty set ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["linear-fused", "linear-reference-sequence", "westervelt-fused"])
def test_no_points_change_nothing(which):
    """``point_source=None`` and a ``PointSources`` without points: no launch is added, and the fields are equal bit for bit.  The mesh
    is the 40 x 1 x 1 row of tests/test_sponge_gpu.py::test_empty_layer_changes_nothing, for the reason its docstring gives (no entry
    of b receives more than two float-atomic addends, so two runs of the same launches give the same bits)."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, nls, src = pkg("boxmesh"), pkg("linear_solver"), pkg("nonlinear_solver"), pkg("sources")
    mesh = boxmesh.BoxMesh(2, (40, 1, 1), length=(0.04, 0.001, 0.001), perturb=0.1, seed=3)
    h = ls.time_step_parameters(mesh, 2, 1500.0, F0, 0.04)
    dt, tf, _ = ls.snap_time_step(h, 2, 1500.0, F0, 0.04)
    res = []
    for points in (None, src.PointSources(np.zeros((0, 3)))):
        if which == "westervelt-fused":
            s = nls.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=1500.0, source_frequency=F0, fused=True, point_source=points)
        else:
            s = ls.LinearSpectral3D(mesh, np.float64, fused=which == "linear-fused", point_source=points)
        assert (s._points is None) == (points is None) and (points is None or s._points.npoints == 0)
        s.init()
        s.rk4(0.0, tf, dt, max_steps=6)
        res.append((s.u_sol(), s.v_sol()))
    assert np.max(np.abs(res[0][0])) > 0
    assert np.array_equal(res[1][0].view(np.int64), res[0][0].view(np.int64)) and np.array_equal(res[1][1].view(np.int64), res[0][1].view(np.int64))


# ---- hipGraph replay -----------------------------------------------------------------------------------------------------------------
def test_graph_replay_with_points_is_refused():
    """The point sources' stage time is a host argument of their launch: rk4_graph raises instead of replaying a stale time."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, lib_mod = pkg("boxmesh"), pkg("linear_solver"), pkg("_lib")
    mesh = boxmesh.BoxMesh(2, (3, 3, 3), length=0.006)
    s = ls.LinearSpectral3D(mesh, np.float64, point_source=_two_points(mesh, 1e-8))
    s.init()
    with pytest.raises(lib_mod.FusGpuError, match="point_source"):
        s.rk4_graph(0.0, 1e-6, 1e-7, max_steps=2)
    assert not hasattr(s, "_graphs") and not np.any(s.u_sol())


# ---- fp32 ----------------------------------------------------------------------------------------------------------------------------
def test_fp32_linear_solver_with_points():
    """The fused fp32 solver driven by two points (facet source silenced) against the fp64 one.  The bar is the solver's own fp32
    error: twice the fp32-to-fp64 distance of the FACET-SOURCE run on the same mesh and steps, measured here (the rule of
    tests/test_sponge_gpu.py::test_fp32_linear_solver_with_layer).

    The mesh is the 6 x 3 x 3 box at P = 4 with cells of 2^-9 m, so that every vertex is exact in fp32 and the fp32 and the fp64 run
    solve the SAME problem: a point is located in the mesh of the solver's own type, and on a box of 12 x 6 x 6 mm the fp32 rounding
    of the vertices (7e-10 m) moves the point by 4e-7 of a cell, its Lagrange rows by 1e-6 -- a different source, not an error of the
    arithmetic (measured there on one MI355X: facet source 7.88e-08, 1.88e-07; point sources 7.49e-07, 5.36e-07).  Measured on this
    mesh, rel l2 (u, v): facet source 1.16e-07, 1.99e-07; point sources 1.62e-07, 2.35e-07 (bars 2.32e-07, 3.98e-07)."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, sensors = pkg("boxmesh"), pkg("linear_solver"), pkg("sensors")
    k = dict(_LINEAR["box"], length=(6 * 2.0**-9, 3 * 2.0**-9, 3 * 2.0**-9))
    meshes = {np.dtype(ft).name: boxmesh.BoxMesh(k["P"], k["cells"], length=k["length"], dtype=ft) for ft in (np.float64, np.float32)}
    mesh = meshes["float64"]
    assert np.array_equal(meshes["float32"].x_g.astype(np.float64), mesh.x_g)
    h = ls.time_step_parameters(mesh, k["P"], 1500.0, F0, mesh.length[0])
    dt, tf, _ = ls.snap_time_step(h, k["P"], 1500.0, F0, mesh.length[0])
    ps = _two_points(mesh, dt)
    assert np.array_equal(sensors.sensor_setup(meshes["float32"], ps.points).weights, sensors.sensor_setup(mesh, ps.points).weights)
    out = {}
    for points in (False, True):
        for ft in (np.float64, np.float32):
            kw = dict(point_source=ps, source_amplitude=0.0) if points else {}
            s = ls.LinearSpectral3D(meshes[np.dtype(ft).name], ft, **kw)
            s.init()
            s.rk4(0.0, tf, dt, max_steps=k["steps"])
            out[points, np.dtype(ft).name] = (s.u_sol().astype(np.float64), s.v_sol().astype(np.float64))
    facet = [rel_l2(out[False, "float32"][i], out[False, "float64"][i]) for i in (0, 1)]
    point = [rel_l2(out[True, "float32"][i], out[True, "float64"][i]) for i in (0, 1)]
    print(f"fp32 to fp64, rel l2 (u, v): facet source {facet[0]:.3e} {facet[1]:.3e}, point sources {point[0]:.3e} {point[1]:.3e}")
    assert np.max(np.abs(out[True, "float64"][0])) > 0 and min(facet) > 0
    assert point[0] < 2 * facet[0] and point[1] < 2 * facet[1]
