"""Relaxation mechanisms on the GPU: the streaming kernel (csrc/relaxation.hpp) against numpy in every kind, both wave solvers -- every
stage implementation -- against the CPU model (tests/relaxation_cpu.py), partitioned runs, hipGraph replay, the plane-wave
absorption and dispersion against the theory, the absorbed power, the guards, and ``relaxation=None``."""

import numpy as np
import pytest

import relaxation_cpu
from conftest import pkg, rel_l2
from oracle import rk4_oracle
from test_relaxation import PLANE_WAVE_ALPHA_BOUND, PLANE_WAVE_SPEED_BOUND

pytestmark = pytest.mark.gpu

_lockstep = pkg("solver_base").run_lockstep
A_RUNGE, B_RUNGE = (0.0, 0.5, 0.5, 1.0), (1 / 6, 1 / 3, 1 / 3, 1 / 6)


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
def _numpy_stage(kind, bw, aw, aw_u, itau, kd, x0, xn, acc, ub, vn):
    """The table of csrc/relax_table.hpp in numpy (fp64): returns the arrays after the pass and ur."""
    x0, xn, acc = x0.copy(), xn.copy(), acc.copy()
    k = kd * vn - (x0 if kind == 0 else xn) * itau[:, None]
    if kind == 2:
        x0 = acc + bw * k
        nxt = x0
    else:
        acc = (x0 if kind == 0 else acc) + bw * k
        xn = x0 + aw * k
        nxt = xn
    ur = ub + aw_u * vn
    for row in nxt:
        ur = ur + row
    return x0, xn, acc, ur


def _relax_stage_case(dtype, nr, n, offsets=(0, 1), mode=None, perdofs=(False, True), kinds=(0, 1, 2), odd_stride=False, figures=None):
    """The launches of ``test_relax_stage_kernel`` on ``n`` owned dofs and their checks; ``mode``: ``TUNE_VECTOR_STREAM`` for the
    launches (None: as it stands); ``odd_stride``: one more entry per row (rows that do not start 16-byte aligned).  Returns
    {(offset, perdof, kind): (x0, xn, acc, ur) as the launch left them}; ``figures`` collects the largest error over its bound."""
    if mode is None:
        return _relax_stage_launches(dtype, nr, n, offsets, perdofs, kinds, odd_stride, figures)
    lib = pkg("_lib")
    before_mode = lib.get_tuning(lib.TUNE_VECTOR_STREAM)
    lib.set_tuning(lib.TUNE_VECTOR_STREAM, mode)
    try:
        return _relax_stage_launches(dtype, nr, n, offsets, perdofs, kinds, odd_stride, figures)
    finally:
        lib.set_tuning(lib.TUNE_VECTOR_STREAM, before_mode)


def _relax_stage_launches(dtype, nr, n, offsets, perdofs, kinds, odd_stride, figures):
    import torch

    torch.cuda.set_device(0)
    ops = pkg("operators")
    tdt = torch.from_numpy(np.zeros(1, dtype)).dtype
    eps = np.finfo(dtype).eps
    w = 16 // np.dtype(dtype).itemsize
    stride, nlocal = -(-(n + 3) // w) * w + int(odd_stride), n  # a few entries past nlocal in every row
    rng = np.random.default_rng(1000 * nr + n)
    tau = rng.uniform(0.5, 2.0, nr)
    itau = (1.0 / tau).astype(dtype).astype(np.float64)  # the kernel rounds 1 / tau to the field's type
    ks = rng.uniform(0.2, 1.0, nr)
    bw, aw, aw_u = (float(dtype(x)) for x in (0.31, 0.47, 0.23))
    host = {name: rng.uniform(0.5, 2.0, (nr, stride)).astype(dtype) * rng.choice([-1.0, 1.0], (nr, stride)).astype(dtype)
            for name in ("x0", "xn", "acc")}
    kd = rng.uniform(0.2, 1.0, (nr, stride)).astype(dtype)
    ub, vn, ur0 = (rng.uniform(0.5, 2.0, n + 2).astype(dtype) for _ in range(3))

    def dev(a, offset):  # the array at an element offset into its own allocation (allocations are 256-byte aligned)
        buf = torch.zeros(a.size + offset, dtype=tdt, device="cuda")
        view = buf[offset:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 256 == offset * a.itemsize
        return view

    results = {}
    for offset in offsets:
        for perdof in perdofs:
            for kind in kinds:
                d = {k_: dev(v_, offset) for k_, v_ in host.items()}
                kd_d, ub_d, vn_d, ur_d = dev(kd, offset), dev(ub, offset), dev(vn, offset), dev(ur0, offset)
                au = 0.0 if kind == 2 else aw_u
                ops.relax_stage(bw, aw, au, kind, tau, kd_d if perdof else ks, d["x0"], d["xn"], d["acc"], ub_d, vn_d, ur_d, nlocal)
                torch.cuda.synchronize()
                weights = kd[:, :n].astype(np.float64) if perdof else np.repeat(ks.astype(dtype).astype(np.float64)[:, None], n, axis=1)
                ref = _numpy_stage(kind, bw, aw, au, itau, weights, *(host[k_][:, :n].astype(np.float64) for k_ in ("x0", "xn", "acc")),
                                   ub[:n].astype(np.float64), vn[:n].astype(np.float64))
                got = [d[k_].cpu().numpy() for k_ in ("x0", "xn", "acc")] + [ur_d.cpu().numpy()]
                what = f"{np.dtype(dtype).name} NR {nr} n {n} offset {offset} perdof {perdof} kind {kind}"
                for name, g, r, before in zip(("x0", "xn", "acc"), got[:3], ref[:3], (host["x0"], host["xn"], host["acc"])):
                    assert np.max(np.abs(g[:, :n] - r)) <= 16 * eps * max(1.0, np.max(np.abs(r))), (what, name)
                    assert np.array_equal(g[:, n:].view(np.uint8), before[:, n:].view(np.uint8)), (what, name, "padding")
                    written = name == "x0" if kind == 2 else name in ("xn", "acc")
                    assert written != np.array_equal(g[:, :n].view(np.uint8), before[:, :n].view(np.uint8)), (what, name, "written")
                assert np.max(np.abs(got[3][:n] - ref[3])) <= 16 * eps * max(1.0, np.max(np.abs(ref[3]))), (what, "ur")
                assert np.array_equal(got[3][n:].view(np.uint8), ur0[n:].view(np.uint8)), (what, "ur past nlocal")
                assert np.array_equal(ub_d.cpu().numpy().view(np.uint8), ub.view(np.uint8)) and np.array_equal(vn_d.cpu().numpy().view(np.uint8), vn.view(np.uint8))
                results[offset, perdof, kind] = got
                if figures is not None:
                    figures[offset, perdof, kind] = max(float(np.max(np.abs(g[..., :n] - r)) / (16 * eps * max(1.0, np.max(np.abs(r)))))
                                                        for g, r in zip(got, ref))
    return results


@pytest.mark.parametrize("n", [1, 7, 1027, 65541])
@pytest.mark.parametrize("nr", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_relax_stage_kernel(dtype, nr, n):
    """FIRST, MIDDLE and LAST, scalar and per-dof weights, operands 256-byte aligned and every one of them one element further (the
    W = 1 form), on arrays filled with nonzero values: against numpy in fp64, to round-off of the type (every output is a sum of at
    most 3 + NR terms of size <= 4: 16 eps of the largest); what a kind does not write, the row padding and the entries past nlocal
    keep their bits."""
    _relax_stage_case(dtype, nr, n)


def test_relax_stage_argument_checks():
    import torch

    torch.cuda.set_device(0)
    ops, lib_mod = pkg("operators"), pkg("_lib")
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    tau, ks = [1e-7, 2e-7], [0.1, 0.1]
    ok = lambda: (z(2, 8), z(2, 8), z(2, 8), z(8), z(8), z(8))  # noqa: E731
    ops.relax_stage(0.1, 0.1, 0.1, 0, tau, ks, *ok(), 8)
    with pytest.raises(TypeError):
        ops.relax_stage(0.1, 0.1, 0.1, 0, tau, ks, z(2, 8), z(2, 8), z(2, 8, dt=torch.float32), z(8), z(8), z(8), 8)
    with pytest.raises(ValueError):
        ops.relax_stage(0.1, 0.1, 0.1, 0, tau, ks, z(3, 8), z(3, 8), z(3, 8), z(8), z(8), z(8), 8)  # three rows, two times
    with pytest.raises(ValueError):
        ops.relax_stage(0.1, 0.1, 0.1, 0, tau, ks, *ok(), 9)  # nlocal > stride
    with pytest.raises(ValueError):
        ops.relax_stage(0.1, 0.1, 0.1, 0, tau, ks, z(2, 8), z(2, 8), z(2, 8), z(8), z(7), z(8), 8)
    with pytest.raises(ValueError):
        ops.relax_stage(0.1, 0.1, 0.1, 3, tau, ks, *ok(), 8)
    with pytest.raises(ValueError):
        ops.relax_stage(0.1, 0.1, 0.1, 0, tau, z(2, 4), *ok(), 8)  # per-dof weights of another shape
    with pytest.raises(lib_mod.FusGpuError):
        ops.relax_stage(0.1, 0.1, 0.1, 0, tau, ks, z(2, 8), z(2, 8), z(2, 8), z(8).cpu(), z(8), z(8), 8)  # no CPU path
    with pytest.raises(lib_mod.FusGpuError):
        ops.relax_stage(0.1, 0.1, 0.1, 0, [1e-7, 0.0], ks, *ok(), 8)  # the entry point refuses tau <= 0


# ---- time loops against the CPU model ----------------------------------------------------------------------------------------------
_MESHES = {"P2-2x2x2": dict(P=2, cells=(2, 2, 2), seed=5), "P3-3x2x2": dict(P=3, cells=(3, 2, 2), seed=6)}
_TAU = {1: np.array([8e-7]), 3: np.array([8e-7, 3e-7, 1.6e-6])}
_STEPS, _L = 20, 0.006
_cache = {}


def _tissue_weights(mesh, nr, L=_L):
    """Per-cell weights that jump between cells: two tissues by the cell centroid in the box of edge ``L`` (the same function of
    position on every rank)."""
    cen = mesh.x_g.astype(np.float64)[mesh.x_dofs].mean(axis=1)
    soft = (cen[:, 0] > 0.5 * L) ^ (cen[:, 1] > 0.5 * L)
    base = np.array([0.06, 0.03, 0.09])[:nr]
    return np.where(soft[None, :], base[:, None], 0.25 * base[:, None])


def _mesh_case(name):
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    if name not in _cache:
        k = _MESHES[name]
        mesh = boxmesh.BoxMesh(k["P"], k["cells"], length=_L, perturb=0.1, seed=k["seed"])
        h = ls.time_step_parameters(mesh, k["P"], 1500.0, 0.5e6, _L)
        dt = ls.snap_time_step(h, k["P"], 1500.0, 0.5e6, _L)[0]
        _cache[name] = (mesh, dt, 1000 * dt)  # a final time no run here reaches: max_steps ends them
    return _cache[name]


def _model_case(name, which, nr, oracle_c):
    """The CPU model's fields for a mesh, a solver and a mechanism count -- computed once, read-only -- and the loss-free oracle's."""
    key = (name, which, nr)
    if key not in _cache:
        mesh, dt, _ = _mesh_case(name)
        kc = _tissue_weights(mesh, nr)
        assert len(np.unique(kc[0])) == 2
        if which == "linear":
            ref = relaxation_cpu.solve(mesh, _STEPS, dt, _TAU[nr], kc, oracle_c=oracle_c)
            free = rk4_oracle.solve(mesh, _STEPS, dt, oracle_c=oracle_c)
        else:
            ref = relaxation_cpu.solve_westervelt(mesh, _STEPS, dt, _TAU[nr], kc, c0=1500.0, f0=0.5e6, oracle_c=oracle_c)
            free = rk4_oracle.solve_westervelt(mesh, _STEPS, dt, c0=1500.0, f0=0.5e6, oracle_c=oracle_c)
        for a in ref + free:
            a.setflags(write=False)
        _cache[key] = (kc, ref, free)
    return _cache[key]


def _solver(which, mesh, relaxation, **kw):
    ls, nls = pkg("linear_solver"), pkg("nonlinear_solver")
    if which == "linear":
        return ls.LinearSpectral3D(mesh, np.float64, relaxation=relaxation, **kw)
    kw.setdefault("fused", True)
    return nls.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=1500.0, source_frequency=0.5e6, relaxation=relaxation, **kw)


@pytest.mark.parametrize("nr", [1, 3])
@pytest.mark.parametrize("which", ["linear", "westervelt"])
@pytest.mark.parametrize("name", list(_MESHES))
def test_solvers_with_mechanisms_match_model(oracle_c, name, which, nr):
    """20 steps with per-cell weights that jump between cells: the fused stage with the lean vector pass, with the reference's stage
    kinds (FUS_RK4_LEAN=0) and the reference launch sequence, each against the CPU model at the bar of tests/test_sponge_gpu.py (1e-11
    in u, v; the memory variables to the same bar against the size of u); fused against fused=False at the bar of the parent's
    fused-versus-reference-sequence test (1e-12); and the mechanisms are not a no-op."""
    import torch

    torch.cuda.set_device(0)
    rx = pkg("relaxation")
    mesh, dt, tf = _mesh_case(name)
    kc, (u_ref, v_ref, xi_ref), (u_free, _) = _model_case(name, which, nr, oracle_c)
    got = {}
    for variant in ("fused-lean", "fused-reference-kinds", "reference-sequence"):
        s = _solver(which, mesh, rx.RelaxationAbsorption(_TAU[nr], kc), fused=variant != "reference-sequence")
        if variant == "fused-reference-kinds":
            s.lean_stages = False
        assert s.lean_stages == (variant != "fused-reference-kinds") and s._relax.kappa.shape[0] == nr
        s.init()
        _, steps = s.rk4(0.0, tf, dt, max_steps=_STEPS)
        assert steps == _STEPS
        u, v = s.u_sol(), s.v_sol()
        xi = s._relax.xi0[:, : s.nlocal].cpu().numpy()
        du, dv, dx = rel_l2(u, u_ref), rel_l2(v, v_ref), float(np.linalg.norm(xi - xi_ref) / np.linalg.norm(u_ref))
        print(f"{name} {which} NR {nr} {variant}: rel l2 to the model u {du:.3e} v {dv:.3e} xi {dx:.3e}; to the loss-free oracle u {rel_l2(u, u_free):.3e}")
        assert np.max(np.abs(u_ref)) > 0 and np.max(np.abs(xi_ref)) > 0
        assert du < 1e-11 and dv < 1e-11 and dx < 1e-11
        assert rel_l2(u, u_free) > 1e-4
        got[variant] = (u, v)
    for variant in ("fused-lean", "fused-reference-kinds"):
        assert rel_l2(got[variant][0], got["reference-sequence"][0]) < 1e-12 and rel_l2(got[variant][1], got["reference-sequence"][1]) < 1e-12


def test_state_persists_across_rk4_calls(oracle_c):
    """Two rk4() calls of 10 steps equal one of 20: the memory variables (and ur) carry over; init() zeroes them."""
    import torch

    torch.cuda.set_device(0)
    rx = pkg("relaxation")
    mesh, dt, tf = _mesh_case("P2-2x2x2")
    kc, (u_ref, v_ref, _), _ = _model_case("P2-2x2x2", "linear", 3, oracle_c)
    for fused in (True, False):
        s = _solver("linear", mesh, rx.RelaxationAbsorption(_TAU[3], kc), fused=fused)
        s.init()
        t, _ = s.rk4(0.0, tf, dt, max_steps=10)
        s.rk4(t, tf, dt, max_steps=10)
        assert rel_l2(s.u_sol(), u_ref) < 1e-11 and rel_l2(s.v_sol(), v_ref) < 1e-11
        s.init()
        assert not torch.any(s._relax.xi0) and not torch.any(s._relax.ur)
        s.rk4(0.0, tf, dt, max_steps=_STEPS)
        assert rel_l2(s.u_sol(), u_ref) < 1e-11


def test_scalar_weights_keep_no_per_dof_vector(oracle_c):
    """Homogeneous weights [NR]: the bound state holds the host scalars, and the fields equal the model's."""
    import torch

    torch.cuda.set_device(0)
    rx = pkg("relaxation")
    mesh, dt, tf = _mesh_case("P2-2x2x2")
    kappa = np.array([0.05, 0.02, 0.08])
    u_ref, v_ref, _ = relaxation_cpu.solve(mesh, _STEPS, dt, _TAU[3], kappa, oracle_c=oracle_c)
    s = _solver("linear", mesh, rx.RelaxationAbsorption(_TAU[3], kappa))
    assert isinstance(s._relax.kappa, np.ndarray) and s._relax.kappa_cells is None
    s.init()
    s.rk4(0.0, tf, dt, max_steps=_STEPS)
    assert rel_l2(s.u_sol(), u_ref) < 1e-11 and rel_l2(s.v_sol(), v_ref) < 1e-11


# ---- two in-process ranks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["linear-fused", "linear-reference-sequence", "westervelt-fused"])
def test_partitioned_solvers_with_mechanisms(variant):
    """Two ranks sharing cuda:0 in this process on 4 x 2 x 2 cells split across x, per-cell weights that jump at the partition boundary
    and across y; the set-up exchange (with the reverse exchanges of the weights' lumped projection) deferred to the driver.  Against
    the single-rank run by lexicographic id over the owned dofs: only if ur -- not u_n -- is what travels do the ghost entries the
    stiffness apply reads carry the memory variables of the neighbour's dofs."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, scat, utils, rx = pkg("boxmesh"), pkg("linear_solver"), pkg("scatterer"), pkg("utils"), pkg("relaxation")
    which, fused = ("westervelt", True) if variant == "westervelt-fused" else ("linear", variant == "linear-fused")
    P, cells, L, R, nsteps, nr = 3, (4, 2, 2), 0.012, 2, 8, 3
    meshes = [boxmesh.BoxMesh(P, cells, grid=(2, 1, 1), rank=r, length=L) for r in range(R)]
    serial = boxmesh.BoxMesh(P, cells, length=L)
    h = ls.time_step_parameters(serial, P, 1500.0, 0.5e6, L)
    dt, tf, _ = ls.snap_time_step(h, P, 1500.0, 0.5e6, L)
    one = _solver(which, serial, rx.RelaxationAbsorption(_TAU[nr], _tissue_weights(serial, nr, L)), fused=fused)
    free = _solver(which, serial, None, fused=fused)
    for s in (one, free):
        s.init()
        s.rk4(0.0, tf, dt, max_steps=nsteps)
    u_one, v_one = one.u_sol(), one.v_sol()
    xi_one = one._relax.xi0[:, : one.nlocal].cpu().numpy()
    assert rel_l2(u_one, free.u_sol()) > 1e-4
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    wid = 8300 + ["linear-fused", "linear-reference-sequence", "westervelt-fused"].index(variant)
    solvers = [_solver(which, meshes[r], rx.RelaxationAbsorption(_TAU[nr], _tissue_weights(meshes[r], nr, L)), fused=fused,
                       comm=scat.NativeComm(local=(wid, R, r)), halo_plan=(od[r], gd[r]), defer_setup_exchange=True) for r in range(R)]
    assert all(s._relax is None for s in solvers)  # nothing is bound before the set-up exchange
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        s.init()
    res = _lockstep([s.rk4_schedule(0.0, tf, dt, max_steps=nsteps) for s in solvers])
    torch.cuda.synchronize()
    assert all(r[1] == nsteps for r in res) and np.max(np.abs(u_one)) > 0
    seen = np.zeros(u_one.size, dtype=int)
    for m, s in zip(meshes, solvers):
        lex = m.global_lexicographic_ids()[: m.nlocal]
        seen[lex] += 1
        assert rel_l2(s.u_sol(), u_one[lex]) < 1e-11 and rel_l2(s.v_sol(), v_one[lex]) < 1e-11
        xi = s._relax.xi0[:, : s.nlocal].cpu().numpy()
        assert np.linalg.norm(xi - xi_one[:, lex]) < 1e-11 * np.linalg.norm(u_one)
        assert s.halo.health() == 0
    assert np.all(seen == 1)


def test_unbound_mechanisms_are_an_error():
    """A solver whose deferred set-up exchange was never run has no state: stepping it raises instead of skipping the mechanisms."""
    import torch

    torch.cuda.set_device(0)
    rx, lib_mod = pkg("relaxation"), pkg("_lib")
    mesh, dt, tf = _mesh_case("P2-2x2x2")
    s = _solver("linear", mesh, rx.RelaxationAbsorption([8e-7], [0.05]), defer_setup_exchange=True)
    with pytest.raises(lib_mod.FusGpuError, match="set-up exchange"):
        s.init()


# ---- hipGraph replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["linear", "westervelt"])
def test_graph_replay_with_mechanisms_matches_rk4(which):
    """rk4_graph with mechanisms: the pass takes fixed pointers and constants only and is captured with the step -- the replayed
    steps (and the shorter last one through rk4) equal rk4's at the existing replay bar (1e-13); the mechanisms were in the captured
    step; the memory variables agree too."""
    import torch

    torch.cuda.set_device(0)
    rx = pkg("relaxation")
    mesh, dt, _ = _mesh_case("P3-3x2x2")
    tf = 14.5 * dt  # 14 full steps and a shorter last one
    kc = _tissue_weights(mesh, 3)
    a, b, free = (_solver(which, mesh, r) for r in (rx.RelaxationAbsorption(_TAU[3], kc), rx.RelaxationAbsorption(_TAU[3], kc), None))
    for s in (a, b, free):
        s.init()
    ta, sa = a.rk4(0.0, tf, dt)
    t1, s1 = b.rk4_graph(0.0, tf, dt, max_steps=6)  # captures
    t2, s2 = b.rk4_graph(t1, tf, dt)  # replays the same graph, then the short last step
    free.rk4_graph(0.0, tf, dt)
    assert sa == 15 and s1 == 6 and s1 + s2 == sa and abs(t2 - ta) < 1e-18 and len(b._graphs) == 1
    assert np.max(np.abs(a.u_sol())) > 0
    assert rel_l2(b.u_sol(), a.u_sol()) < 1e-13 and rel_l2(b.v_sol(), a.v_sol()) < 1e-13
    assert rel_l2(b._relax.xi0.cpu().numpy(), a._relax.xi0.cpu().numpy()) < 1e-13 and torch.any(a._relax.xi0)
    assert rel_l2(b.u_sol(), free.u_sol()) > 1e-4


# ---- the guards on the device ------------------------------------------------------------------------------------------------------
def test_time_step_guard_in_every_loop():
    """dt / min(tau) >= 2.785: rk4, rk4_schedule and rk4_graph raise ValueError before any step."""
    import torch

    torch.cuda.set_device(0)
    rx = pkg("relaxation")
    mesh, dt, tf = _mesh_case("P2-2x2x2")
    s = _solver("linear", mesh, rx.RelaxationAbsorption([dt / 2.8, 8e-7], [0.01, 0.01]))
    s.init()
    for loop in (lambda: s.rk4(0.0, tf, dt, max_steps=2), lambda: next(s.rk4_schedule(0.0, tf, dt, max_steps=2)),
                 lambda: s.rk4_graph(0.0, tf, dt, max_steps=2)):
        with pytest.raises(ValueError, match="2.785"):
            loop()
    assert not torch.any(s.u0) and not torch.any(s.u)
    s.rk4(0.0, tf, 0.99 * dt, max_steps=2)  # dt / min(tau) = 2.772, below the limit: runs


# ---- relaxation=None ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["linear-fused", "linear-reference-sequence", "westervelt-fused", "westervelt-reference-sequence"])
def test_without_mechanisms_nothing_changes(which):
    """``relaxation=None`` against a solver built without the keyword: u and v after 10 steps bit for bit, and no state is kept.  A row
    of cells (40 x 1 x 1, as the empty-layer test of tests/test_sponge_gpu.py): no entry of b receives more than two float-atomic addends,
    so two runs of the same launches give the same bits."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, nls = pkg("boxmesh"), pkg("linear_solver"), pkg("nonlinear_solver")
    mesh = boxmesh.BoxMesh(2, (40, 1, 1), length=(0.04, 0.001, 0.001), perturb=0.1, seed=3)
    h = ls.time_step_parameters(mesh, 2, 1500.0, 0.5e6, 0.04)
    dt, tf, _ = ls.snap_time_step(h, 2, 1500.0, 0.5e6, 0.04)
    res = []
    for kw in ({}, {"relaxation": None}):
        fused = which.endswith("-fused")
        if which.startswith("westervelt"):
            s = nls.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=1500.0, source_frequency=0.5e6, fused=fused, **kw)
        else:
            s = ls.LinearSpectral3D(mesh, np.float64, fused=fused, **kw)
        assert s.relaxation is None and s._relax is None and len(s._graph_state()) == 7
        s.init()
        s.rk4(0.0, tf, dt, max_steps=10)
        res.append((s.u_sol(), s.v_sol()))
    assert np.max(np.abs(res[0][0])) > 0
    assert np.array_equal(res[1][0].view(np.int64), res[0][0].view(np.int64)) and np.array_equal(res[1][1].view(np.int64), res[0][1].view(np.int64))


# ---- the physics on the device: absorption, dispersion, absorbed power -------------------------------------------------------------
def _plane_wave_run():
    """The plane-wave experiment of tests/test_relaxation.py on the device, once: the fused linear solver, a FieldMonitor of the
    fundamental over the last period."""
    if "plane" not in _cache:
        import torch

        torch.cuda.set_device(0)
        ls, fm = pkg("linear_solver"), pkg("field_monitor")
        k = relaxation_cpu.plane_wave_case()
        s = ls.LinearSpectral3D(k["mesh"], np.float64, speed_of_sound=k["c"], source_frequency=k["f0"], relaxation=k["model"])
        mon = fm.FieldMonitor(s.nlocal, np.float64, harmonics=(1,), frequency=k["f0"])
        s.init()
        nsteps = k["per"] * k["periods"]
        tf = nsteps * k["dt"]
        _, steps = s.rk4(0.0, tf + 0.5 * k["dt"], k["dt"], max_steps=nsteps, monitor=mon, record_from=(k["periods"] - 1) / k["f0"] + 0.5 * k["dt"])
        assert steps == nsteps and mon.nacc == k["per"]
        _cache["plane"] = (k, s, mon)
    return _cache["plane"]


def test_plane_wave_absorption_and_dispersion_on_the_device():
    """The fitted log-amplitude slope of the fundamental against alpha_r(w0) and its phase slope against c_ph(w0), with the CPU
    test's bounds (twice the CPU model's own deviation on this mesh: 4.05 % and 2.6e-5)."""
    k, s, mon = _plane_wave_run()
    model, w0 = k["model"], 2 * np.pi * k["f0"]
    x = k["mesh"].dof_coordinates()[: s.nlocal, 0]
    alpha, kx = relaxation_cpu.fit_slopes(x, mon.harmonic_amplitude(1).cpu().numpy(), mon.harmonic_phase(1).cpu().numpy(), *k["x_fit"])
    alpha_r, c_ph = model.alpha(k["f0"], k["c"]), model.phase_speed(k["f0"], k["c"])
    da, dc = alpha / alpha_r - 1.0, (w0 / kx) / c_ph - 1.0
    print(f"plane wave, device: alpha {alpha:.5f} against {alpha_r:.5f} ({da:+.3e}), speed {w0 / kx:.4f} against {c_ph:.4f} ({dc:+.3e})")
    assert abs(da) <= PLANE_WAVE_ALPHA_BOUND and abs(dc) <= PLANE_WAVE_SPEED_BOUND


def test_heat_deposition_of_the_plane_wave():
    """``relaxation.heat_deposition`` on that wave equals alpha_total |P_1|^2 / (rho c) -- 2 alpha I of a plane wave; the linear
    solver has no delta, so alpha_total = alpha_r(w0) -- at the interior dofs, within the absorption test's bound; and the solver
    without mechanisms is refused."""
    rx = pkg("relaxation")
    k, s, mon = _plane_wave_run()
    q = rx.heat_deposition(mon, s).cpu().numpy()
    x = k["mesh"].dof_coordinates()[: s.nlocal, 0]
    inner = (x >= k["x_fit"][0]) & (x <= k["x_fit"][1])
    p1 = mon.harmonic_amplitude(1).cpu().numpy()
    expect = k["model"].alpha(k["f0"], k["c"]) * p1**2 / (s.rho0 * k["c"])
    assert inner.sum() > 100 and np.min(expect[inner]) > 0
    dev = np.max(np.abs(q[inner] / expect[inner] - 1.0))
    print(f"heat deposition against alpha |P_1|^2 / (rho c) at {inner.sum()} interior dofs: largest relative deviation {dev:.3e}")
    assert dev <= PLANE_WAVE_ALPHA_BOUND
    # and it is the power the wave loses: -dI/dx = 2 alpha I with the FITTED alpha, I = |P_1|^2 / (2 rho c)
    alpha_fit, _ = relaxation_cpu.fit_slopes(x, p1, mon.harmonic_phase(1).cpu().numpy(), *k["x_fit"])
    assert np.max(np.abs(q[inner] / (alpha_fit * p1[inner] ** 2 / (s.rho0 * k["c"])) - 1.0)) <= PLANE_WAVE_ALPHA_BOUND
    with pytest.raises(ValueError, match="relaxation"):
        rx.heat_deposition(mon, pkg("linear_solver").LinearSpectral3D(_mesh_case("P2-2x2x2")[0], np.float64))
