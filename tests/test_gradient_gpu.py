"""The gradient cell operator on the device (csrc/gradient_geom.hpp through operators.gradient_operator) against its numpy restatement
(tests/gradient_cpu.py, anchored to the reference's data in tests/test_gradient.py), and the maps of intensity.py: through solvers of
every stiffness form, from a monitor's harmonics end to end, and on 2 / 4 in-process ranks."""
import numpy as np
import pytest

import gradient_cpu as gc
from conftest import TOL, pkg, ref_field, rel_l2, rel_max
from test_sensors_gpu import _bowl, _linear, _lockstep, _mesh, _westervelt

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 16, -7.25

# cells per degree: not a multiple of cells_per_batch(P) (64, 28, 16, 10, 7, 5, 4, 3, 2, 2 for P = 1 .. 10: every degree the operator
# dispatches) and at least two batches, so that the last batch is partial and dofs are shared between batches
SHAPES = {1: (5, 4, 4), 2: (4, 3, 3), 3: (4, 3, 3), 4: (3, 2, 2), 5: (4, 2, 2), 6: (3, 2, 2), 7: (3, 3, 1), 8: (7, 1, 1), 9: (3, 3, 1),
          10: (3, 3, 1)}


def _np(t):
    return t.detach().cpu().numpy()


def _case(P, shape, dtype, shuffle=False):
    """Inputs of one case, rounded to ``dtype`` once: the device and the restatement (fp64 arithmetic) read the same numbers."""
    mesh = pkg("boxmesh").BoxMesh(P, shape, perturb=0.16, seed=P)
    pts, wts, D = pkg("gll").tabulate_1d(P, dtype)
    rng = np.random.default_rng(100 + P)
    x = ref_field(mesh.dof_coordinates()).astype(dtype)
    cc = (0.5 + rng.random(mesh.ncells)).astype(dtype)
    dofmap, x_dofs = np.asarray(mesh.dofmap), np.asarray(mesh.x_dofs)
    if shuffle:  # a cell order without locality: the plan cache keeps the plan with a cell order of its own (ORDERED)
        perm = rng.permutation(mesh.ncells)
        dofmap, x_dofs, cc = np.ascontiguousarray(dofmap[perm]), np.ascontiguousarray(x_dofs[perm]), np.ascontiguousarray(cc[perm])
    x_g = np.asarray(mesh.x_g).astype(dtype)
    add = gc.weak_gradient(x_dofs, x_g, pts, wts, D, dofmap, x, cc, mesh.ndofs)  # what the operator adds
    # y3 is pre-filled with values a tenth the size of what is added: large enough to be missed if overwritten, too small to hide an error
    y0 = (0.1 * np.sqrt(np.mean(add**2)) * rng.standard_normal((3, mesh.ndofs))).astype(dtype)
    ref = y0.astype(np.float64) + add
    return dict(P=P, dtype=dtype, ndofs=mesh.ndofs, ncells=mesh.ncells, x=x, cc=cc, y0=y0, dofmap=dofmap, x_dofs=x_dofs, x_g=x_g,
                pts=pts, wts=wts, D=D, ref=ref, add=add)


_CASES = {}


def _cached_case(P, shape, dtype, shuffle=False):
    key = (P, shape, np.dtype(dtype).name, shuffle)
    if key not in _CASES:
        _CASES[key] = _case(P, shape, dtype, shuffle)
    return _CASES[key]


def _apply(c):
    """One launch into a [3, ndofs] view of a buffer whose rows are GUARD elements longer (ystride > ndofs); returns y3 on the host and
    whether every guard element still holds the sentinel."""
    import torch

    ops = pkg("operators")
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    op = ops.gradient_operator(c["P"], c["D"].flatten(), c["dtype"], geometry=(c["x_dofs"], c["x_g"], c["pts"], c["wts"]))
    n = c["ndofs"]
    buf = torch.full((3, n + GUARD), SENTINEL, dtype=td(c["x"]).dtype, device="cuda")
    y3 = buf[:, :n]
    y3.copy_(td(c["y0"]))
    dm = td(c["dofmap"])
    op.prepare(dm)
    op(td(c["x"]), td(c["cc"]), y3, dm)
    torch.cuda.synchronize()
    return _np(y3), bool((buf[:, n:] == SENTINEL).all().item())


def _check(got, ref, dtype, what):
    tol = TOL[np.dtype(dtype)]
    for d in range(3):
        l2, mx = rel_l2(got[d], ref[d]), rel_max(got[d], ref[d])
        print(f"{what} component {d}: rel l2 {l2:.3e} max {mx:.3e}")
        assert l2 <= tol["l2"] and mx <= tol["mx"], f"{what} component {d}: rel l2 {l2:.3e}, max {mx:.3e}"


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("P", sorted(SHAPES))
def test_operator_equals_the_restatement(P, dtype):
    import torch

    torch.cuda.set_device(0)
    lib = pkg("_lib").load()
    c = _cached_case(P, SHAPES[P], dtype)
    cpb = lib.fus_plan_entities_per_batch((P + 1) ** 3)
    assert c["ncells"] % cpb != 0 and c["ncells"] > cpb  # a partial last batch, at least two batches
    got, guards = _apply(c)
    assert guards, "the launch wrote behind a component of y3"
    assert np.max(np.abs(got - c["y0"])) > 0.5 * np.max(np.abs(c["add"])) and np.max(np.abs(c["y0"])) > 0  # it ADDED to the pre-filled y3
    _check(got, c["ref"], dtype, f"P={P} {np.dtype(dtype).name}")


# cells per degree for the shuffled order: more than 2 cells_per_batch(P), which is where the plan cache tries a cell order
ORDERED_SHAPES = {2: (4, 4, 4), 4: (3, 3, 3), 6: (3, 2, 2)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("runs", [0, 2], ids=["lists", "run-tables"])
@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "ordered"])
@pytest.mark.parametrize("P", sorted(ORDERED_SHAPES))
def test_all_four_plan_shapes(P, ordered, runs, dtype):
    """(ORDERED, RUNS): a shuffled cell order makes the plan cache keep a plan with a cell order of its own; the run tables are
    switched off and on through the tuning switch the other planned operators use."""
    import torch

    torch.cuda.set_device(0)
    ops, lib = pkg("operators"), pkg("_lib")
    c = _cached_case(P, ORDERED_SHAPES[P], dtype, shuffle=ordered)
    old_runs, old_loc = lib.get_tuning(lib.TUNE_PLAN_RUNS), ops._LOCALITY_ORDER
    try:
        lib.set_tuning(lib.TUNE_PLAN_RUNS, runs)  # 0: never (the plan is built without tables), 2: every launch reads them
        ops.use_locality_order(True)
        ops._PLANS.clear()
        got, guards = _apply(c)
        assert (ops._PLANS.last_order is not None) == ordered
    finally:
        lib.set_tuning(lib.TUNE_PLAN_RUNS, old_runs)
        ops.use_locality_order(old_loc)
        ops._PLANS.clear()
    assert guards
    _check(got, c["ref"], dtype, f"P={P} ordered={ordered} runs={runs} {np.dtype(dtype).name}")


@pytest.mark.parametrize("form", ["affine", "G-stream-P2", "in-kernel-P4"])
def test_recovered_gradient_of_a_linear_field_whatever_the_stiffness_form(form):
    import torch

    torch.cuda.set_device(0)
    ls, it = pkg("linear_solver"), pkg("intensity")
    L = 0.012
    if form == "affine":
        solver = ls.LinearSpectral3D(_mesh("affine", 3, L), np.float64)
        assert solver.affine
    elif form == "G-stream-P2":
        solver = ls.LinearSpectral3D(_mesh("perturbed", 2, L), np.float64, in_kernel_geometry=False)
        assert not solver.affine and not solver.in_kernel_geometry
    else:
        solver = ls.LinearSpectral3D(_mesh("perturbed", 4, L), np.float64)
        assert solver.in_kernel_geometry
    a = np.array([1.3, -0.7, 2.1])
    u = torch.from_numpy(solver.mesh.dof_coordinates() @ a + 0.01).cuda()
    g = _np(it.recovered_gradient(solver, u))
    assert g.shape == (3, solver.nlocal) and g.dtype == np.float64
    err = np.max(np.abs(g - a[:, None]))
    print(f"{form}: max error {err:.3e}")
    assert err <= 1e-11 * np.linalg.norm(a)
    assert it._gradient_operator(solver) is solver._gradient_op  # built once, kept on the solver
    g_owned = _np(it.recovered_gradient(solver, u[: solver.nlocal].contiguous()))
    assert np.array_equal(g_owned, g) or np.max(np.abs(g_owned - g)) <= 1e-12 * np.linalg.norm(a)


def test_intensity_and_radiation_force_from_a_monitor():
    """A Westervelt run on a bowl mesh, harmonics (1, 2) over its fifth period: the maps equal the restatement fed the monitor's own sums."""
    import torch

    torch.cuda.set_device(0)
    fm, it = pkg("field_monitor"), pkg("intensity")
    P, L = 3, 0.012
    mesh = _mesh("bowl", P, L)
    s, dt_stable, tf = _westervelt(mesh, True, P, L)
    period = 1.0 / s.f0
    # 8 steps per period: the stable step of this coarse mesh is half a period, and two samples per period see no imaginary part of the
    # first harmonic (sin(k w t) = 0 at both), i.e. no intensity at all
    K = 8
    dt = period / K
    assert dt <= dt_stable
    m = fm.FieldMonitor(s.nlocal, np.float64, harmonics=(1, 2), frequency=s.f0)
    # four periods for the wave to enter the box (its source is ramped up over them), then one period recorded
    s.rk4(0.0, tf, dt, max_steps=5 * K, monitor=m, record_from=(4 * K + 0.5) * dt)
    assert m.nacc == K
    pts, wts, D = pkg("gll").tabulate_1d(P)
    geo = gc.Geometry.of_mesh(mesh, pts, wts, D)
    omega = 2.0 * np.pi * s.f0
    harm = []
    for k in (1, 2):
        hre, him = m._harmonic(k)
        harm.append((k, omega, 2.0 / K * _np(hre), 2.0 / K * _np(him)))
    assert max(np.max(np.abs(h[2])) for h in harm) > 0.0
    I_ref = sum(gc.intensity_of(geo, k, w, re, im, s.rho_cells) for k, w, re, im in harm)
    F_ref = gc.radiation_force(geo, harm, s.delta_cells, s.rho_cells, s.c_cells)
    tol = TOL[np.dtype(np.float64)]
    for name, got, ref in (("intensity", m.intensity(s), I_ref), ("radiation force", m.radiation_force(s), F_ref),
                           ("intensity of harmonic 2", it.intensity(m, s, harmonics=(2,)), gc.intensity_of(geo, *harm[1], s.rho_cells))):
        got = _np(got)
        assert got.shape == (3, s.nlocal)
        print(f"{name}: rel l2 {rel_l2(got, ref):.3e} max {rel_max(got, ref):.3e}, max |ref| {np.max(np.abs(ref)):.3e}")
        assert np.max(np.abs(ref)) > 0.0 and rel_l2(got, ref) <= tol["l2"] and rel_max(got, ref) <= tol["mx"], name
    vre, vim = it.particle_velocity(m, s, 1)
    rre, rim = gc.particle_velocity(geo, *harm[0], s.rho_cells)
    assert rel_l2(_np(vre), rre) <= tol["l2"] and rel_l2(_np(vim), rim) <= tol["l2"]
    # |I| goes through the existing focus
    foc = fm.focus(it.magnitude(m.intensity(s)), s, 0.5)
    assert foc["max"] == pytest.approx(float(np.max(np.sqrt((I_ref**2).sum(axis=0)))), rel=1e-10) and 0 < foc["volume"] <= 1.3 * L**3
    with pytest.raises(ValueError):
        it.radiation_force(m, _linear(mesh, True, P, L)[0])  # no absorption model


@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 1)], ids=["2ranks", "4ranks"])
def test_partitioned_maps_equal_the_single_rank_maps(grid):
    """2 / 4 ranks sharing cuda:0 in this process (the pattern of tests/test_field_monitor_gpu.py): each rank's owned dofs of
    ``recovered_gradient`` and ``intensity`` are the single-rank maps; interface dofs get contributions from cells of two ranks."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, scat, utils, fm, it = (pkg(n) for n in ("boxmesh", "linear_solver", "scatterer", "utils", "field_monitor", "intensity"))
    P, cells, L, K = 3, (4, 4, 4), 0.012, 6
    R = int(np.prod(grid))
    warp = _bowl(L, cells[0])
    meshes = [boxmesh.BoxMesh(P, cells, grid=grid, rank=r, length=L, ghost_order=5, warp=warp) for r in range(R)]
    serial = boxmesh.BoxMesh(P, cells, length=L, warp=warp)
    h = ls.time_step_parameters(serial, P, 1500.0, 0.5e6, L)
    dt, tf, _ = ls.snap_time_step(h, P, 1500.0, 0.5e6, L)
    monitor = lambda s: fm.FieldMonitor(s.nlocal, np.float64, harmonics=(1, 2), frequency=s.f0)  # noqa: E731
    field = lambda mesh: torch.from_numpy(ref_field(mesh.dof_coordinates() / L)).cuda()  # noqa: E731
    cc = lambda mesh: 1.0 + 0.3 * np.sin(40.0 * np.asarray(mesh.x_g)[np.asarray(mesh.x_dofs)].mean(axis=1).sum(axis=1))  # noqa: E731  (per cell, by position)

    one = ls.LinearSpectral3D(serial, np.float64)
    one.init()
    m1 = monitor(one)
    one.rk4(0.0, tf, dt, max_steps=K, monitor=m1, record_from=1.5 * dt)
    lex1 = serial.global_lexicographic_ids()[: serial.nlocal]
    nglob = serial.nlocal
    ref_g, ref_i = np.zeros((3, nglob)), np.zeros((3, nglob))
    ref_g[:, lex1] = _np(it.recovered_gradient(one, field(serial), cc(serial)))
    ref_i[:, lex1] = _np(it.intensity(m1, one))
    assert np.max(np.abs(ref_i)) > 0.0

    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    wid = 7900 + 10 * R
    solvers = [ls.LinearSpectral3D(meshes[r], np.float64, comm=scat.NativeComm(local=(wid, R, r)), halo_plan=(od[r], gd[r]),
                                   defer_setup_exchange=True) for r in range(R)]
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        s.init()
    monitors = [monitor(s) for s in solvers]
    _lockstep([s.rk4_schedule(0.0, tf, dt, K, monitor=mo, record_from=1.5 * dt) for s, mo in zip(solvers, monitors)])
    # the field over the OWNED dofs only: the ghosts come from the forward exchange
    grads = _lockstep([it.recovered_gradient_schedule(s, field(s.mesh)[: s.nlocal].contiguous(), cc(s.mesh)) for s in solvers])
    intens = _lockstep([it.intensity_schedule(mo, s) for s, mo in zip(solvers, monitors)])
    torch.cuda.synchronize()
    for s in solvers:
        s.check_halo_health("test")
    got_g, got_i, count = np.zeros((3, nglob)), np.zeros((3, nglob)), np.zeros(nglob, dtype=np.int64)
    for mesh, g, i in zip(meshes, grads, intens):
        lex = mesh.global_lexicographic_ids()[: mesh.nlocal]
        count[lex] += 1
        got_g[:, lex], got_i[:, lex] = _np(g), _np(i)
    assert np.array_equal(count, np.ones(nglob, dtype=np.int64))
    assert any(m.ndofs > m.nlocal for m in meshes)  # ghosts: interface dofs receive contributions from cells of another rank
    tol = TOL[np.dtype(np.float64)]
    for name, got, ref in (("recovered gradient", got_g, ref_g), ("intensity", got_i, ref_i)):
        print(f"{name} on {R} ranks: rel l2 {rel_l2(got, ref):.3e} max {rel_max(got, ref):.3e}")
        assert rel_l2(got, ref) <= tol["l2"] and rel_max(got, ref) <= tol["mx"], name


def test_operator_argument_errors_raise_before_any_launch():
    import torch

    torch.cuda.set_device(0)
    ops, lib_mod = pkg("operators"), pkg("_lib")
    c = _cached_case(2, SHAPES[2], np.float64)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    geometry = (c["x_dofs"], c["x_g"], c["pts"], c["wts"])
    op = ops.gradient_operator(2, c["D"].flatten(), np.float64, geometry=geometry)
    x, cc, dm = td(c["x"]), td(c["cc"]), td(c["dofmap"])
    y3 = torch.zeros((3, c["ndofs"]), dtype=torch.float64, device="cuda")
    with pytest.raises(lib_mod.FusGpuError):
        op(x.cpu(), cc, y3, dm)
    with pytest.raises(lib_mod.FusGpuError):
        op(x, cc, y3.cpu(), dm)
    with pytest.raises(TypeError):
        op(x, cc, y3.to(torch.float32), dm)
    with pytest.raises(ValueError):
        op(x, cc, y3[:, :-1], dm)  # rows shorter than x
    with pytest.raises(ValueError):
        op(x, cc, y3.T.contiguous(), dm)  # [ndofs, 3]
    with pytest.raises(ValueError):
        op(x, cc[:-1], y3, dm)
    short = ops.gradient_operator(2, c["D"].flatten(), np.float64, geometry=(c["x_dofs"][:-1],) + geometry[1:])
    with pytest.raises(ValueError, match="x_dofs"):
        short(x, cc, y3, dm)  # x_dofs rows do not match the dofmap's cells
    with pytest.raises(ValueError):
        ops.gradient_operator(2, c["D"].flatten(), np.float64, geometry=(c["x_dofs"], c["x_g"], c["pts"][:-1], c["wts"]))
    torch.cuda.synchronize()
    assert float(y3.abs().max().item()) == 0.0  # nothing was launched
