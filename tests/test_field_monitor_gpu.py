"""Full-field monitors on the device (csrc/field_monitor.hpp through the C ABI and field_monitor.FieldMonitor): the kernel against
numpy, the solvers' ``rk4(..., monitor=...)`` (fused path, reference sequence, hipGraph replay, 2 / 4 in-process ranks), the
derived maps and the bowl demo's ``--field-stats``."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg
from test_sensors_gpu import _linear, _lockstep, _mesh, _points, _westervelt

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7.25
SIZES = (1, 3, 255, 257, 1027)  # the tail alone, one lane, a workgroup boundary - 1 / + 1, several workgroups + tail


def _np(t):
    return t.detach().cpu().numpy()


class _Buffers:
    """u, v and every output of one case on the device, each with GUARD sentinel elements after its n (after every row of
    hre / him); ``shift``: every pointer one element past a 16-byte boundary (the scalar kernel)."""

    def __init__(self, n, dtype, H, shift):
        import torch

        self.n, self.H, self.shift = n, H, shift
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        self.stride = n + GUARD + ((n + GUARD) & 1) + (1 if shift and H else 0)  # even when aligned, odd for the scalar path
        mk = lambda m, dt: torch.full((m + GUARD + 2,), SENTINEL, dtype=dt, device="cuda")[shift: shift + m + GUARD]  # noqa: E731
        self.u, self.v = mk(n, tdt), mk(n, tdt)
        self.pmax, self.pmin = mk(n, tdt), mk(n, tdt)
        self.usq, self.vsq = mk(n, torch.float64), mk(n, torch.float64)
        rows = lambda: torch.full((max(H, 1) * self.stride + 2,), SENTINEL, dtype=torch.float64, device="cuda")[shift: shift + max(H, 1) * self.stride]  # noqa: E731
        self.hre, self.him = rows(), rows()
        for t in (self.u, self.pmax, self.usq, self.hre):
            assert (t.data_ptr() % 16 != 0) == bool(shift)

    def guards_untouched(self):
        for t in (self.pmax, self.pmin, self.usq, self.vsq):
            if not bool((t[self.n:] == SENTINEL).all().item()):
                return False
        for t in (self.hre, self.him):
            r = t.reshape(max(self.H, 1), self.stride)
            if not bool((r[:, self.n:] == SENTINEL).all().item()):
                return False
        return True


def _accumulate(lib, dtype, b, outs, u, v, coef, init, launched=None):
    import torch

    fn = getattr(lib, "fus_field_accumulate_" + ("f64" if dtype == np.float64 else "f32"))
    b.u[: b.n].copy_(torch.from_numpy(u))
    b.v[: b.n].copy_(torch.from_numpy(v))
    cd = torch.from_numpy(np.ascontiguousarray(coef)).cuda() if coef is not None else None
    on = lambda name, t: t.data_ptr() if name in outs else None  # noqa: E731
    H = b.H if "harm" in outs else 0
    if launched is not None:  # the H this launch is called with: the instantiation it dispatches
        launched.append(H)
    rc = fn(b.u.data_ptr(), b.v.data_ptr() if "vsq" in outs else None, b.n, on("peak", b.pmax), on("peak", b.pmin), on("usq", b.usq),
            on("vsq", b.vsq), on("harm", b.hre), on("harm", b.him), b.stride, cd.data_ptr() if H else None, H, int(init),
            pkg("_lib").stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0


def _window(lib, dtype, b, outs, rng, records, figures=None, launched=None):
    """``records`` records of seeded random (u, v), the first with ``init``; checks every output that is on against numpy, and that
    every output that is off, and every guard element, still holds the sentinel."""
    n, H = b.n, b.H
    us = [(10.0 * rng.standard_normal(n)).astype(dtype) for _ in range(records)]
    vs = [(1e3 * rng.standard_normal(n)).astype(dtype) for _ in range(records)]
    coefs = [rng.uniform(-1.0, 1.0, 2 * H) for _ in range(records)]
    for k in range(records):
        _accumulate(lib, dtype, b, outs, us[k], vs[k], coefs[k] if H else None, k == 0, launched)
    U, V = np.asarray(us, dtype=np.float64), np.asarray(vs, dtype=np.float64)  # an fp32 field converts exactly
    eps = 2.0 ** -52

    def check_sum(got, terms):  # the same sequence in numpy: acc = terms[0]; acc = acc + terms[k] (two roundings where the device has one FMA)
        acc = terms[0].copy()
        for k in range(1, records):
            acc = acc + terms[k]
        bound = 2 * records * eps * np.abs(terms).sum(axis=0)
        err = np.abs(_np(got)[:n] - acc)
        if figures is not None:  # the largest error over its bound
            figures.append(float(np.max(err / bound)))
        assert np.all(err <= bound), (float(err.max()), float(bound.min()))

    if "peak" in outs:
        assert np.array_equal(_np(b.pmax)[:n], np.asarray(us).max(axis=0)) and np.array_equal(_np(b.pmin)[:n], np.asarray(us).min(axis=0))
        assert b.pmax.dtype == b.u.dtype
    else:
        assert bool((b.pmax == SENTINEL).all().item()) and bool((b.pmin == SENTINEL).all().item())
    if "usq" in outs:
        check_sum(b.usq, U * U)
    else:
        assert bool((b.usq == SENTINEL).all().item())
    if "vsq" in outs:
        check_sum(b.vsq, V * V)
    else:
        assert bool((b.vsq == SENTINEL).all().item())
    if "harm" in outs and H:
        re, im = b.hre.reshape(H, b.stride), b.him.reshape(H, b.stride)
        for h in range(H):
            check_sum(re[h], U * np.asarray([c[2 * h] for c in coefs])[:, None])
            check_sum(im[h], U * np.asarray([c[2 * h + 1] for c in coefs])[:, None])
    else:
        assert bool((b.hre == SENTINEL).all().item()) and bool((b.him == SENTINEL).all().item())
    assert b.guards_untouched()


def _output_sets(H):
    return [("peak",), ("usq",), ("vsq",), ("peak", "usq", "vsq", "harm")] + ([("harm",)] if H else [])


def _kernel_case(dtype, H, shift, sizes=SIZES, sets=None, windows=(5, 3), collect=None, figures=None, launched=None):
    """``sets``: the output sets to run (default: all of ``_output_sets``); ``windows``: records per window; ``collect``: a list that
    receives every output buffer, guards included, as the last window of each (size, set) left it; ``figures``: a list that receives
    every sum's largest error as a ratio to its bound; ``launched``: a list that receives the H of every launch (0 for an output set
    without "harm": such a launch runs the H = 0 build whatever the buffers' H)."""
    import torch

    torch.cuda.set_device(0)
    lib = pkg("_lib").load()
    rng = np.random.default_rng(100 * H + shift)
    for n in sizes:
        for outs in (_output_sets(H) if sets is None else sets):
            b = _Buffers(n, dtype, H, shift)
            for records in windows:  # a second window: its first record (init) must not see the first window
                _window(lib, dtype, b, outs, rng, records, figures, launched)
            if collect is not None:
                collect.append([_np(t) for t in (b.pmax, b.pmin, b.usq, b.vsq, b.hre, b.him)])


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("H", [0, 1, 2, 4])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_kernel_against_numpy(dtype, H, shift):
    """Extrema bitwise; sums within 2 N 2^-52 sum|terms| per dof of the same sequence in numpy fp64 (N records: the device contracts
    acc + a b to one FMA where numpy rounds twice, each rounding at most half an ulp of a partial sum bounded by sum|terms|)."""
    _kernel_case(dtype, H, shift)


def test_streaming_build_gives_the_same_results():
    lib = pkg("_lib")
    before = lib.get_tuning(lib.TUNE_VECTOR_STREAM)
    try:
        for mode in (2, 4):  # always: non-temporal loads and stores / stores only
            lib.set_tuning(lib.TUNE_VECTOR_STREAM, mode)
            _kernel_case(np.float64, 4, 0, sizes=(1027,))
            _kernel_case(np.float64, 2, 1, sizes=(1027,))
    finally:
        lib.set_tuning(lib.TUNE_VECTOR_STREAM, before)
    assert lib.get_tuning(lib.TUNE_VECTOR_STREAM) == before


def test_known_signal():
    """16 records over exactly one period of A cos(w t + phi) + B cos(2 w t): the sums are exact and harmonics below 8 do not alias."""
    import torch

    torch.cuda.set_device(0)
    fm = pkg("field_monitor")
    n, N, f0 = 300, 16, 1.1e6
    w = 2 * np.pi * f0
    rng = np.random.default_rng(5)
    m = fm.FieldMonitor(n, np.float64, peak=True, mean_square=("u",), harmonics=(1, 2), frequency=f0)
    with pytest.raises(ValueError):
        m.peak()  # nothing recorded
    for scale in (1.0, 3.0):  # the second window, after reset(), must not see the first
        A, B, phi = scale * rng.uniform(0.5, 2.0, n), scale * rng.uniform(0.1, 1.0, n), rng.uniform(-3.0, 3.0, n)
        series = []
        for k in range(1, N + 1):
            t = k / (N * f0)
            series.append(A * np.cos(w * t + phi) + B * np.cos(2 * w * t))
            m.record(torch.from_numpy(series[-1]).cuda(), None, t)
        assert m.nacc == N
        tol = 1e-12 * A.max()
        assert np.max(np.abs(_np(m.harmonic_amplitude(1)) - A)) <= tol
        assert np.max(np.abs(_np(m.harmonic_amplitude(2)) - B)) <= tol
        assert np.max(np.abs(_np(m.harmonic_phase(1)) - phi)) <= tol
        assert np.max(np.abs(_np(m.mean_square("u")) - 0.5 * (A * A + B * B))) <= tol
        assert np.array_equal(_np(m.peak()[0]), np.max(series, axis=0)) and np.array_equal(_np(m.peak()[1]), np.min(series, axis=0))
        m.reset()
        assert m.nacc == 0
    with pytest.raises(ValueError):
        m.mean_square("v")  # not accumulated
    with pytest.raises(ValueError):
        m.harmonic_amplitude(3)
    mv = fm.FieldMonitor(n, np.float64, mean_square=("v",))
    with pytest.raises(ValueError, match="pass v"):
        mv.record(torch.zeros(n, dtype=torch.float64, device="cuda"), None, 0.0)
    with pytest.raises(TypeError):
        mv.record(torch.zeros(n, dtype=torch.float32, device="cuda"), None, 0.0)
    with pytest.raises(ValueError):
        mv.record(torch.zeros(n - 1, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"), 0.0)


def test_planned_and_ring_records_accumulate_alike():
    """80 records of which only the first 10 are planned (expect_steps): those read the uploaded table, the other 70 = _RING + 6
    the pinned ring, whose first six rows are reused after the wrap.  n = 1027 = 4 * 256 + 3: several workgroups and a tail beyond
    the 16-byte accesses."""
    import torch

    torch.cuda.set_device(0)
    fm, ring = pkg("field_monitor"), pkg("recording")._RING
    n, K, f0 = 1027, 10 + ring + 6, 1.1e6
    rng = np.random.default_rng(23)
    ends = fm.record_times(0.0, 1.0, 0.9e-7 / 7, max_steps=K)  # the step ends of a run: t_0 .. t_79
    us = [10.0 * rng.standard_normal(n) for _ in range(K)]
    vs = [1e3 * rng.standard_normal(n) for _ in range(K)]
    m = fm.FieldMonitor(n, np.float64, peak=True, mean_square=("u", "v"), harmonics=(1, 2), frequency=f0)
    m.expect_steps(0.0, 1.0, 0.9e-7 / 7, max_steps=10)  # a run whose step ends are t_0 .. t_9
    assert np.array_equal(m.factors.planned_times, ends[:10]) and m.factors.planned_left == 10
    for k in range(K):
        m.record(torch.from_numpy(us[k]).cuda(), torch.from_numpy(vs[k]).cuda(), ends[k])
        assert m.factors.planned_left == max(9 - k, 0)  # exhausted after record 9
    assert m.nacc == K
    _assert_statistics(_held(m), _reference_statistics(us, vs, ends, f0))


def test_entry_point_errors_precede_device_work():
    lib = pkg("_lib").load()
    z, one = C.c_void_p(0), C.c_void_p(4096)  # non-null, never dereferenced: validation fails first
    for fn in (lib.fus_field_accumulate_f64, lib.fus_field_accumulate_f32):
        assert fn(one, one, -1, one, one, one, one, one, one, 8, one, 1, 1, z) == -1  # n < 0
        assert fn(one, one, 4, one, one, one, one, one, one, 8, one, -1, 1, z) == -1  # H < 0
        assert fn(one, one, 4, one, one, one, one, one, one, 8, one, 5, 1, z) == -1  # H > 4
        assert fn(one, one, 4, one, one, one, one, z, one, 8, one, 1, 1, z) == -1  # H > 0 without hre
        assert fn(one, one, 4, one, one, one, one, one, z, 8, one, 1, 1, z) == -1  # ... without him
        assert fn(one, one, 4, one, one, one, one, one, one, 8, z, 1, 1, z) == -1  # ... without coef
        assert fn(one, one, 4, one, one, one, one, one, one, 3, one, 1, 1, z) == -1  # hstride < n
        assert fn(one, z, 4, one, one, one, one, one, one, 8, one, 1, 1, z) == -1  # vsq without v
        assert fn(one, one, 4, one, z, one, one, one, one, 8, one, 1, 1, z) == -1  # pmax without pmin
        assert fn(one, one, 4, z, one, one, one, one, one, 8, one, 1, 1, z) == -1  # pmin without pmax
        assert fn(z, z, 4, z, z, one, z, z, z, 0, z, 0, 1, z) == -1  # an output, no field
        assert fn(one, one, 0, one, one, one, one, one, one, 8, one, 1, 1, z) == 0  # n == 0: no-op
        assert fn(z, z, 0, z, z, z, z, z, z, 0, z, 0, 0, z) == 0
        assert fn(one, one, 4, z, z, z, z, z, z, 0, z, 0, 1, z) == 0  # nothing requested: no-op


def _rel(a, b):
    a, b = (np.asarray(_np(x) if hasattr(x, "cpu") else x, dtype=np.float64) for x in (a, b))
    assert a.shape == b.shape
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _monitor(solver, n=None):
    return pkg("field_monitor").FieldMonitor(solver.nlocal if n is None else n, np.float64, peak=True, mean_square=("u", "v"),
                                             harmonics=(1, 2), frequency=solver.f0)


def _reference_statistics(us, vs, ends, f0):
    """numpy statistics of the recorded steps: what a FieldMonitor with peak, both mean squares and harmonics (1, 2) holds."""
    sens = pkg("sensors")
    U, V = np.asarray(us), np.asarray(vs)
    coef = np.asarray([sens.harmonic_coefficients((1, 2), 2 * np.pi * f0, t) for t in ends])  # [K, 4]
    return {"pmax": U.max(axis=0), "pmin": U.min(axis=0), "usq": (U * U).sum(axis=0), "vsq": (V * V).sum(axis=0),
            "hre": np.stack([(U * coef[:, 2 * h, None]).sum(axis=0) for h in range(2)]),
            "him": np.stack([(U * coef[:, 2 * h + 1, None]).sum(axis=0) for h in range(2)])}


def _held(m):
    n = m.nlocal
    return {"pmax": _np(m._pmax), "pmin": _np(m._pmin), "usq": _np(m._usq), "vsq": _np(m._vsq), "hre": _np(m._hre)[:, :n],
            "him": _np(m._him)[:, :n]}


def _assert_statistics(got, ref, tol=1e-11):
    for k, r in ref.items():
        assert np.max(np.abs(r)) > 0, k
        assert np.max(np.abs(got[k] - r)) <= tol * np.max(np.abs(r)), k


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
@pytest.mark.parametrize("solver", ["linear", "westervelt"])
def test_solver_accumulates_the_recorded_steps(solver, fused):
    """rk4(..., monitor=m, record_from=...) over 6 steps against the same run taken one rk4(max_steps=1) call at a time with u_sol() /
    v_sol() after each and numpy statistics over steps 3 .. 6.  Separate runs are compared to the project's fp64 tolerance: the
    stiffness flush adds with float atomics, whose order varies from run to run."""
    import torch

    torch.cuda.set_device(0)
    sens = pkg("sensors")
    L, K = 0.012, 6
    P, kind, make = (3, "perturbed", _linear) if solver == "linear" else (2, "bowl", _westervelt)
    mesh = _mesh(kind, P, L)
    a, dt, tf = make(mesh, fused, P, L)
    m = _monitor(a)
    assert a.rk4(0.0, tf, dt, max_steps=K, monitor=m, record_from=2.5 * dt)[1] == K
    assert m.nacc == K - 2
    b, _, _ = make(mesh, fused, P, L)
    tb, us, vs, ends = 0.0, [], [], []
    for k in range(K):
        tb, _ = b.rk4(tb, tf, dt, max_steps=1)
        if k >= 2:
            us.append(b.u_sol().copy()), vs.append(b.v_sol().copy()), ends.append(tb)
    ref = _reference_statistics(us, vs, ends, a.f0)
    _assert_statistics(_held(m), ref)
    assert _rel(m.mean_square("v"), ref["vsq"] / (K - 2)) <= 1e-11
    assert _rel(m.harmonic_amplitude(2), 2.0 / (K - 2) * np.hypot(ref["hre"][1], ref["him"][1])) <= 1e-11
    # the run itself is the run without a monitor
    c, _, _ = make(mesh, fused, P, L)
    c.rk4(0.0, tf, dt, max_steps=K)
    assert _rel(a.u, c.u) <= 1e-11 and _rel(a.v, c.v) <= 1e-11
    # monitor and sensors together share record_from; the sensor series are those of sensors alone
    pts = _points(mesh, L, np.random.default_rng(3), m=40)
    d, _, _ = make(mesh, fused, P, L)
    sd, md = sens.PointSensors(mesh, pts, np.float64, capacity=K), _monitor(d)
    d.rk4(0.0, tf, dt, max_steps=K, sensors=sd, monitor=md, record_from=2.5 * dt)
    e, _, _ = make(mesh, fused, P, L)
    se = sens.PointSensors(mesh, pts, np.float64, capacity=K)
    e.rk4(0.0, tf, dt, max_steps=K, sensors=se, record_from=2.5 * dt)
    assert sd.nrec == se.nrec == md.nacc == K - 2
    assert _rel(sd.series(), se.series()) <= 1e-11
    _assert_statistics(_held(md), ref)
    # the plan of recorded steps is the sensors' plan
    assert np.array_equal(md.factors.planned_times, record_plan(sens, mesh, pts, a.f0, tf, dt, K, 2.5 * dt))


def record_plan(sens, mesh, pts, f0, tf, dt, K, rf):
    s = sens.PointSensors(mesh, pts, np.float64, harmonics=(1,), frequency=f0)
    s.expect_steps(0.0, tf, dt, K, rf)
    return s.factors.planned_times


@pytest.mark.parametrize("solver", ["linear", "westervelt"])
def test_graph_replay_accumulates_like_rk4(solver):
    import torch

    torch.cuda.set_device(0)
    P, L, K = 3, 0.006, 7
    mesh = pkg("boxmesh").BoxMesh(P, (4, 3, 3), length=L, perturb=0.1, seed=1)
    make = _linear if solver == "linear" else _westervelt
    a, dt, tf = make(mesh, True, P, L)
    ma = _monitor(a)
    a.rk4(0.0, tf, dt, max_steps=K, monitor=ma, record_from=1.5 * dt)
    b, _, _ = make(mesh, True, P, L)
    mb = _monitor(b)
    assert b.rk4_graph(0.0, tf, dt, max_steps=K, monitor=mb, record_from=1.5 * dt)[1] == K
    assert ma.nacc == mb.nacc == K - 1
    _assert_statistics(_held(mb), _held(ma))
    assert _rel(a.u, b.u) <= 1e-11


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 1)], ids=["2ranks", "4ranks"])
def test_partitioned_maps_equal_the_single_rank_maps(grid, fused):
    """2 / 4 ranks sharing cuda:0 in this process: each rank's owned maps, scattered through the global lexicographic ids, are the
    single-rank maps; every global dof is covered exactly once; the merged focus is the single-rank focus."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, scat, utils, fm = pkg("boxmesh"), pkg("linear_solver"), pkg("scatterer"), pkg("utils"), pkg("field_monitor")
    P, cells, L, K = 3, (4, 4, 4), 0.012, 6
    R = int(np.prod(grid))
    meshes = [boxmesh.BoxMesh(P, cells, grid=grid, rank=r, length=L, ghost_order=5) for r in range(R)]
    serial = boxmesh.BoxMesh(P, cells, length=L)
    h = ls.time_step_parameters(serial, P, 1500.0, 0.5e6, L)
    dt, tf, _ = ls.snap_time_step(h, P, 1500.0, 0.5e6, L)
    one = ls.LinearSpectral3D(serial, np.float64, fused=fused)
    one.init()
    m1 = _monitor(one)
    one.rk4(0.0, tf, dt, max_steps=K, monitor=m1, record_from=1.5 * dt)
    lex1 = serial.global_lexicographic_ids()[: serial.nlocal]
    nglob = serial.nlocal
    ref = {k: np.zeros(v.shape[:-1] + (nglob,)) for k, v in _held(m1).items()}
    for k, v in _held(m1).items():
        ref[k][..., lex1] = v
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    wid = 7700 + 10 * R + int(fused)
    solvers = [ls.LinearSpectral3D(meshes[r], np.float64, comm=scat.NativeComm(local=(wid, R, r)), fused=fused,
                                   halo_plan=(od[r], gd[r]), defer_setup_exchange=True) for r in range(R)]
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        s.init()
    monitors = [_monitor(s) for s in solvers]
    res = _lockstep([s.rk4_schedule(0.0, tf, dt, K, monitor=mo, record_from=1.5 * dt) for s, mo in zip(solvers, monitors)])
    vols = _lockstep([fm.dof_volumes_schedule(s) for s in solvers])
    torch.cuda.synchronize()
    for s in solvers:
        s.check_halo_health("test")
    assert all(r[1] == K for r in res) and all(mo.nacc == K - 1 == m1.nacc for mo in monitors)
    got = {k: np.zeros_like(v) for k, v in ref.items()}
    count = np.zeros(nglob, dtype=np.int64)
    for mesh, mo in zip(meshes, monitors):
        lex = mesh.global_lexicographic_ids()[: mesh.nlocal]
        count[lex] += 1
        for k, v in _held(mo).items():
            got[k][..., lex] = v
    assert np.array_equal(count, np.ones(nglob, dtype=np.int64))
    _assert_statistics(got, ref)
    # the volumes are the single-rank volumes, and the focus of the peak map merges to the single-rank focus
    v1 = np.zeros(nglob)
    v1[lex1] = _np(fm.dof_volumes(one))
    vr = np.zeros(nglob)
    for mesh, v in zip(meshes, vols):
        vr[mesh.global_lexicographic_ids()[: mesh.nlocal]] = _np(v)
    assert np.max(np.abs(vr - v1)) <= 1e-12 * np.max(v1) and abs(v1.sum() - L**3) <= 1e-12 * L**3
    f1 = fm.focus(m1.peak()[0], one, 0.5)
    merged = fm.FieldMonitor.merge_focus([fm.focus(mo.peak()[0], s, 0.5) for s, mo in zip(solvers, monitors)])
    assert abs(merged["max"] - f1["max"]) <= 1e-11 * abs(f1["max"]) and f1["max"] == float(ref["pmax"].max())
    # (the wave of this box is plane: the maximum is attained, to rounding, on a whole y-z plane of dofs, and which of them wins is
    # decided by the last bits -- the x of the focus is what the two runs share)
    assert abs(merged["position"][0] - f1["position"][0]) <= 1e-12 * L and 0 <= merged["rank"] < R
    assert abs(merged["volume"] - f1["volume"]) <= 1e-11 * f1["volume"] and 0 < f1["volume"] < L**3
    assert f1["volume"] == pytest.approx(float(v1[ref["pmax"] >= 0.5 * f1["max"]].sum()), rel=1e-12)
    assert fm.merge_focus([f1])["volume"] == pytest.approx(f1["volume"], rel=1e-14)


def test_heat_deposition(oracle_c):
    """q = M(kappa) <v^2> / M(1) 1 with kappa = delta / (rho c^4): kappa <v^2> in a homogeneous medium; with two materials split at a
    cell plane, the oracle's mass applies of <v^2> with kappa and of ones, divided."""
    import torch

    torch.cuda.set_device(0)
    nls, fm = pkg("nonlinear_solver"), pkg("field_monitor")
    P, L, K = 2, 0.012, 5
    mesh = _mesh("bowl", P, L)
    a, dt, tf = _westervelt(mesh, True, P, L)
    m = fm.FieldMonitor(a.nlocal, np.float64, mean_square=("v",))
    a.rk4(0.0, tf, dt, max_steps=K, monitor=m, record_from=1.5 * dt)
    q, vsq = _np(m.heat_deposition(a)), _np(m.mean_square("v"))
    kappa = a.delta / a.rho0 / a.c0**4
    assert np.max(vsq) > 0 and np.max(np.abs(q - kappa * vsq)) <= 1e-12 * np.max(kappa * vsq)
    with pytest.raises(ValueError):
        fm.heat_deposition(m, _linear(mesh, True, P, L)[0])  # no absorption model
    # two materials: the cells behind the plane x = L / 3 are denser, faster and absorb more
    behind = np.asarray(mesh.x_g)[np.asarray(mesh.x_dofs)].mean(axis=1)[:, 0] > L / 3
    assert 0 < behind.sum() < mesh.ncells
    c = np.where(behind, 2800.0, 1480.0)
    rho = np.where(behind, 1850.0, 1000.0)
    att = np.where(behind, 4.0, 0.2)
    b = nls.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=c, density=rho, attenuation_coefficient_dB=att, fused=True)
    b.init()
    mb = fm.FieldMonitor(b.nlocal, np.float64, mean_square=("v",))
    b.rk4(0.0, tf, dt, max_steps=K, monitor=mb, record_from=1.5 * dt)
    vsq = _np(mb.mean_square("v"))
    kap = nls.compute_diffusivity_of_sound(b.w0, c, att) / rho / c**4
    detJ, dofmap = _np(b.detJ), np.asarray(mesh.dofmap)
    num, den = np.zeros(mesh.ndofs), np.zeros(mesh.ndofs)
    oracle_c.mass_apply(vsq, kap, num, detJ, dofmap)
    oracle_c.mass_apply(np.ones(mesh.ndofs), np.ones(mesh.ncells), den, detJ, dofmap)
    ref = num / den
    assert np.max(ref) > 0 and np.max(np.abs(_np(mb.heat_deposition(b)) - ref)) <= 1e-12 * np.max(ref)


def test_bowl_demo_field_stats_cover_one_period(tmp_path):
    out = os.path.join(tmp_path, "maps.npz")
    P, N, L = 3, 4, 0.004
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fenicsx-fus-gpu_amd", "demo_nonlinear_bowl.py"), "--degree", str(P), "--cells", str(N),
                        "--length", str(L), "--field-stats", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Solve time per step" in r.stdout, r.stdout + r.stderr
    lines = {ln.split(":")[0]: ln.split(":")[1].strip() for ln in r.stdout.splitlines() if ln.startswith("Number of")}
    spp, ndofs = int(lines["Number of steps per period"]), int(lines["Number of degrees-of-freedom"])
    with np.load(out) as z:
        assert int(z["nacc"]) == spp == int(z["steps_per_period"])
        for k in ("pmax", "pmin", "H1", "H2", "q", "u_mean_square"):
            assert z[k].shape == (ndofs,) and np.all(np.isfinite(z[k])), k
        assert np.all(z["pmax"] >= z["pmin"]) and z["pmax"].max() > 1.0 and z["pmin"].min() < -1.0
        assert np.all(z["H1"] >= 0) and np.all(z["q"] >= 0) and z["q"].max() > 0
        assert z["H1"].max() > z["H2"].max() > 0  # a weakly nonlinear wave
        assert float(z["focus_max"]) == z["H1"].max() and z["H1"][int(z["focus_dof"])] == z["H1"].max()
        assert np.all(z["focus_position"] >= -1e-12) and np.all(z["focus_position"] <= 1.2 * L)
        assert 0 < float(z["focus_volume"]) <= 1.001 * L**3
        assert np.array_equal(np.sort(z["lexicographic_ids"]), np.arange(ndofs))
