"""Nodal material fields on the GPU: the stiffness apply with a per-dof coefficient and the geometry formed in the kernel
(csrc/stiffness_geom_nodal.hpp) against the CPU model (tests/nodal_cpu.py: the oracle's apply on the pre-scaled G), its plan shapes,
its algebraic properties and the pre-scaled general-G route; ``LinearSpectral3D(nodal_medium=...)`` -- every stage implementation --
against the CPU loop, partitioned, with the attachments, and replayed from a hipGraph."""

import numpy as np
import pytest

import nodal_cpu
import point_source_cpu
import sponge_cpu
from conftest import TOL, build_problem, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

_lockstep = pkg("solver_base").run_lockstep
F0 = 0.5e6


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    torch.cuda.set_device(0)
    return pkg("device"), pkg("operators")


def _check(got, ref, dtype, what):
    tol = TOL[np.dtype(dtype)]
    e2, em = rel_l2(got, ref), rel_max(got, ref)
    print(f"{what}: rel l2 {e2:.3e} rel max {em:.3e}")
    assert e2 < tol["l2"] and em < tol["mx"], f"{what}: rel l2 {e2:.3e} (tol {tol['l2']}), rel max {em:.3e}"


# ---- the operator ------------------------------------------------------------------------------------------------------------------
_problems = {}


def _problem(P, cells, dtype=np.float64):
    """A perturbed (non-affine) box, a smooth positive kappa with a 3 : 1 range, random per-cell constants, and the CPU model's
    ``y0 + K(cc kappa) x`` -- computed once per case, read-only."""
    key = (P, cells, np.dtype(dtype).name)
    if key not in _problems:
        pb = build_problem(P, cells, dtype=dtype, perturb=0.2, seed=40 + P)
        mesh = pb["mesh"]
        kappa = nodal_cpu.smooth_field(mesh.dof_coordinates(), 1.0, 3.0, 1.0).astype(dtype)
        assert kappa.min() > 0 and kappa.max() / kappa.min() > 2.5
        y0 = np.random.default_rng(P).standard_normal(mesh.ndofs).astype(dtype)
        y_ref = y0.copy()
        nodal_cpu.stiffness_apply(P, pb["D"], pb["x"], pb["cc"], y_ref, pb["G"], mesh.dofmap, kappa)
        for a in (y0, y_ref):
            a.setflags(write=False)
        pb.update(kappa=kappa, y0=y0, y_ref=y_ref)
        _problems[key] = pb
    return _problems[key]


def _nodal_operator(ops, pb, dtype, kappa=None, x_dofs=None):
    mesh = pb["mesh"]
    return ops.stiffness_operator(pb["P"], pb["D"].flatten(), dtype, geometry=(mesh.x_dofs if x_dofs is None else x_dofs, mesh.x_g, pb["pts"], pb["wts"]),
                                  nodal=pb["kappa"] if kappa is None else kappa)


_CASES = [(P, (3, 2, 2), np.float64) for P in range(1, 11)] + [(2, (4, 3, 3), np.float64)] + [(P, (3, 2, 2), np.float32) for P in (2, 4, 6)]


@pytest.mark.parametrize("P,cells,dtype", _CASES, ids=[f"P{P}-{'x'.join(map(str, c))}-{np.dtype(d).name}" for P, c, d in _CASES])
def test_operator_matches_cpu_model(gpu, P, cells, dtype):
    """y += K(cc kappa) x on top of a nonzero y, against the oracle's apply on G kappa[dofmap]: every degree on 3 x 2 x 2 cells (fp64),
    P = 2 on 36 cells (more than one batch of 28, with a tail), fp32 at P = 2, 4, 6."""
    dev, ops = gpu
    pb = _problem(P, cells, dtype)
    mesh = pb["mesh"]
    op = _nodal_operator(ops, pb, dtype)
    assert op.nodal.numel() == mesh.ndofs and op.nodal.is_cuda
    y = dev.to_device(pb["y0"].copy())
    op(dev.to_device(pb["x"]), dev.to_device(pb["cc"]), y, None, dev.to_device(mesh.dofmap))
    _check(y.copy_to_host(), pb["y_ref"], dtype, f"nodal stiffness P={P} {cells} {np.dtype(dtype).name}")
    assert rel_l2(y.copy_to_host(), pb["y0"]) > 1e-2  # the apply added something


def test_operator_argument_checks(gpu):
    dev, ops = gpu
    pb = _problem(2, (3, 2, 2))
    mesh = pb["mesh"]
    x, cc, dm = dev.to_device(pb["x"]), dev.to_device(pb["cc"]), dev.to_device(mesh.dofmap)
    y = dev.to_device(np.zeros(mesh.ndofs))
    with pytest.raises(ValueError, match="one value per dof"):
        _nodal_operator(ops, pb, np.float64, kappa=pb["kappa"][:-1])(x, cc, y, None, dm)
    with pytest.raises(ValueError, match="nodal_medium.scale_G"):
        ops.stiffness_operator(2, pb["D"].flatten(), np.float64, nodal=pb["kappa"])
    op = _nodal_operator(ops, pb, np.float32)  # the coefficient takes the operator's type
    assert op.nodal.dtype == pkg("_lib").torch_dtype(np.float32)
    with pytest.raises(TypeError):
        op(x, cc, y, None, dm)


def test_plan_shapes(gpu):
    """P = 4, 24 cells: the same apply through an ordered plan (rows of the dofmap, of x_dofs and the constants permuted at random:
    the cache builds the batches in ``locality_cell_order``) and with FUS_TUNE_PLAN_RUNS both ways -- all four (ORDERED, RUNS) builds
    -- equals the plain one to 1e-12."""
    dev, ops = gpu
    lib = pkg("_lib")
    pb = _problem(4, (4, 3, 2))
    mesh = pb["mesh"]
    x = dev.to_device(pb["x"])

    def apply(dofmap, x_dofs, cc):
        y = dev.to_device(np.zeros(mesh.ndofs))
        _nodal_operator(ops, pb, np.float64, x_dofs=x_dofs)(x, dev.to_device(cc), y, None, dev.to_device(dofmap))
        return y.copy_to_host()

    perm = np.random.default_rng(3).permutation(mesh.ncells)
    permuted = tuple(np.ascontiguousarray(a[perm]) for a in (mesh.dofmap, mesh.x_dofs, pb["cc"]))
    natural = (mesh.dofmap, mesh.x_dofs, pb["cc"])
    ops._PLANS.clear()
    try:
        plain = apply(*natural)
        assert ops._PLANS.last_order is None
        _check(plain, pb["y_ref"] - pb["y0"], np.float64, "plain")
        for mode in (1, 0, 2):
            lib.set_tuning(lib.TUNE_PLAN_RUNS, mode)
            for name, arrays in (("natural", natural), ("ordered", permuted)):
                got = apply(*arrays)
                if name == "ordered":
                    assert ops._PLANS.last_order is not None, "the random order must have triggered the locality plan"
                err = rel_l2(got, plain)
                print(f"run-table mode {mode}, {name} plan: rel l2 to the plain apply {err:.3e}")
                assert err < 1e-12
            ops._PLANS.clear()
    finally:
        lib.set_tuning(lib.TUNE_PLAN_RUNS, 1)
        ops._PLANS.clear()


def test_constant_kappa_is_the_per_cell_operator(gpu):
    """kappa == 2.5 everywhere: the per-cell geometry operator with the constants 2.5 cc, to 1e-13 relative (fp64, P = 2, 4, 5, 6: both
    flux forms, factors in registers and formed in the loop)."""
    dev, ops = gpu
    for P in (2, 4, 5, 6):
        pb = _problem(P, (3, 2, 2))
        mesh = pb["mesh"]
        x, dm = dev.to_device(pb["x"]), dev.to_device(mesh.dofmap)
        y, y_cell = dev.to_device(np.zeros(mesh.ndofs)), dev.to_device(np.zeros(mesh.ndofs))
        _nodal_operator(ops, pb, np.float64, kappa=np.full(mesh.ndofs, 2.5))(x, dev.to_device(pb["cc"]), y, None, dm)
        ops.stiffness_operator(P, pb["D"].flatten(), np.float64, geometry=(mesh.x_dofs, mesh.x_g, pb["pts"], pb["wts"]))(
            x, dev.to_device(2.5 * pb["cc"]), y_cell, None, dm)
        err = rel_l2(y.copy_to_host(), y_cell.copy_to_host())
        print(f"P={P}: constant kappa against the per-cell operator, rel l2 {err:.3e}")
        assert np.max(np.abs(y_cell.copy_to_host())) > 0 and err < 1e-13


def test_algebraic_properties(gpu):
    """K const = 0 and x.Ky = y.Kx with a nodal coefficient, at the thresholds of tests/test_operators_gpu.py (1e-9 of the size of
    K x; 1e-11 relative)."""
    dev, ops = gpu
    pb = _problem(4, (4, 3, 2))
    mesh = pb["mesh"]
    op, cc, dm = _nodal_operator(ops, pb, np.float64), dev.to_device(pb["cc"]), dev.to_device(mesh.dofmap)

    def K(v):
        y = dev.to_device(np.zeros(mesh.ndofs))
        op(dev.to_device(np.ascontiguousarray(v)), cc, y, None, dm)
        return y.copy_to_host()

    Kx = K(pb["x"])
    scale = np.max(np.abs(Kx))
    k1 = np.max(np.abs(K(np.full(mesh.ndofs, 2.5))))
    v = np.random.default_rng(5).standard_normal(mesh.ndofs)
    a, b = float(v @ Kx), float(pb["x"] @ K(v))
    print(f"|K const| / |K x| = {k1 / scale:.3e}; symmetry {abs(a - b) / max(abs(a), abs(b)):.3e}")
    assert scale > 0 and k1 < 1e-9 * scale
    assert abs(a - b) < 1e-11 * max(abs(a), abs(b))


def test_prescaled_general_route(gpu):
    """The nodal kernel equals the general-G kernel on ``scale_G(G, kappa, dofmap)`` to 1e-12 (P = 3 and 4; P = 2 on 36 cells)."""
    dev, ops = gpu
    nm = pkg("nodal_medium")
    for P, cells in ((3, (3, 2, 2)), (4, (4, 3, 2)), (2, (4, 3, 3))):
        pb = _problem(P, cells)
        mesh = pb["mesh"]
        x, cc, dm = dev.to_device(pb["x"]), dev.to_device(pb["cc"]), dev.to_device(mesh.dofmap)
        Gs = nm.scale_G(dev.to_device(pb["G"]), pb["kappa"], dm)
        assert Gs.is_cuda and Gs.shape == pb["G"].shape
        y, y_g = dev.to_device(np.zeros(mesh.ndofs)), dev.to_device(np.zeros(mesh.ndofs))
        _nodal_operator(ops, pb, np.float64)(x, cc, y, None, dm)
        ops.stiffness_operator(P, pb["D"].flatten(), np.float64)(x, cc, y_g, Gs, dm)
        err = rel_l2(y.copy_to_host(), y_g.copy_to_host())
        print(f"P={P} {cells}: nodal kernel against the general kernel on the pre-scaled G, rel l2 {err:.3e}")
        assert err < 1e-12


# ---- the linear solver -------------------------------------------------------------------------------------------------------------
_P, _CELLS, _L, _STEPS = 3, (4, 2, 2), (0.012, 0.006, 0.006), 20
_C, _RHO = (1500.0, 2400.0), (1000.0, 1800.0)  # water, and the peak of the inclusion
_cache = {}


def _lens_medium(length=_L):
    """A smooth Gaussian inclusion in c and rho at the middle of the box (its tail reaches the source and absorbing faces)."""
    center, radius = 0.5 * np.asarray(length), 0.3 * length[1]
    return pkg("nodal_medium").NodalMedium(nodal_cpu.lens(center, radius, *_C), nodal_cpu.lens(center, radius, *_RHO))


def _solver_mesh(perturbed=True, **kw):
    return pkg("boxmesh").BoxMesh(_P, _CELLS, length=_L, **(dict(perturb=0.1, seed=7) if perturbed else {}), **kw)


def _time_step(mesh):
    ls = pkg("linear_solver")
    h = ls.time_step_parameters(mesh, _P, _C[1], F0, mesh.length[0])
    dt, _, _ = ls.snap_time_step(h, _P, _C[1], F0, mesh.length[0])  # the fastest speed of the medium bounds the step
    return dt, 1000 * dt  # a final time no run here reaches: max_steps ends them


def _solver_case():
    if "plain" not in _cache:
        mesh = _solver_mesh()
        dt, tf = _time_step(mesh)
        c, rho = _lens_medium().evaluate(mesh)
        assert c.max() / c.min() > 1.4 and rho.max() / rho.min() > 1.5
        ref = nodal_cpu.solve(mesh, _STEPS, dt, c, rho, f0=F0)
        for a in ref:
            a.setflags(write=False)
        _cache["plain"] = (mesh, dt, tf, c, rho, ref)
    return _cache["plain"]


@pytest.mark.parametrize("variant", ["fused-lean", "fused-reference-kinds", "reference-sequence", "general-kernel-on-scaled-G"])
def test_linear_solver_with_nodal_medium_matches_model(gpu, variant):
    """20 steps at P = 3 on a perturbed 4 x 2 x 2 box with a smooth lens in c and rho: the fused stage (lean vector pass and the
    reference's stage kinds) and the reference launch sequence, each against the CPU loop to 1e-11; ``in_kernel_geometry=False`` (the
    general kernel on the G array scaled once) gives the same field; and the lens is not a no-op."""
    ls = pkg("linear_solver")
    mesh, dt, tf, c, rho, (u_ref, v_ref) = _solver_case()
    kw = dict(in_kernel_geometry=False) if variant == "general-kernel-on-scaled-G" else {}
    s = ls.LinearSpectral3D(mesh, np.float64, fused=variant != "reference-sequence", nodal_medium=_lens_medium(), **kw)
    if variant == "fused-reference-kinds":
        s.lean_stages = False
    assert s.in_kernel_geometry == (not kw) and (s.stiff.nodal is not None) == (not kw) and not s.affine
    assert np.array_equal(s.c_nodal, c) and np.array_equal(s.rho_nodal, rho)
    assert np.allclose(s.c_cells, c[mesh.dofmap].mean(axis=1)) and np.allclose(s.rho_cells, rho[mesh.dofmap].mean(axis=1))
    fd1 = mesh.facet_dofmap(mesh.boundary_facets([2]))
    assert abs(s.c0 - c[fd1].mean()) < 1e-9
    s.init()
    _, steps = s.rk4(0.0, tf, dt, max_steps=_STEPS)
    assert steps == _STEPS
    u, v = s.u_sol(), s.v_sol()
    du, dv = rel_l2(u, u_ref), rel_l2(v, v_ref)
    if "water" not in _cache:
        w = ls.LinearSpectral3D(mesh, np.float64, speed_of_sound=_C[0], density=_RHO[0])
        w.init()
        w.rk4(0.0, tf, dt, max_steps=_STEPS)
        _cache["water"] = w.u_sol()
    print(f"{variant}: rel l2 to the model u {du:.3e} v {dv:.3e}; to the homogeneous solver u {rel_l2(u, _cache['water']):.3e}")
    assert np.max(np.abs(u_ref)) > 0
    assert du < 1e-11 and dv < 1e-11
    assert rel_l2(u, _cache["water"]) > 1e-3


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
def test_constant_nodal_values_equal_the_scalar_medium(gpu, fused):
    """Constant nodal values -- a scalar, and an array of one value -- against the scalar-medium solver (per-cell constants, the
    per-cell geometry kernel) to 1e-12: stiffness, lumped mass, facet means and the reference speed all reduce to the scalar forms."""
    ls, nm = pkg("linear_solver"), pkg("nodal_medium")
    mesh = _solver_mesh()
    dt, tf = _time_step(mesh)
    ref = ls.LinearSpectral3D(mesh, np.float64, speed_of_sound=1540.0, density=1050.0, fused=fused, in_kernel_geometry=True)
    media = (nm.NodalMedium(1540.0, 1050.0), nm.NodalMedium(np.full(mesh.ndofs, 1540.0), lambda xyz: np.full(xyz.shape[0], 1050.0)))
    runs = [ref] + [ls.LinearSpectral3D(mesh, np.float64, fused=fused, nodal_medium=m) for m in media]
    for s in runs:
        s.init()
        s.rk4(0.0, tf, dt, max_steps=_STEPS)
    assert np.max(np.abs(ref.u_sol())) > 0 and abs(runs[1].c0 - 1540.0) < 1e-9
    for s in runs[1:]:
        du, dv = rel_l2(s.u_sol(), ref.u_sol()), rel_l2(s.v_sol(), ref.v_sol())
        print(f"constant nodal medium against the scalar medium: u {du:.3e} v {dv:.3e}")
        assert du < 1e-12 and dv < 1e-12


def test_solver_argument_conflicts(gpu):
    ls, nm = pkg("linear_solver"), pkg("nodal_medium")
    mesh = _solver_mesh()
    medium = nm.NodalMedium(1500.0, 1000.0)
    with pytest.raises(ValueError, match="nodal_medium"):
        ls.LinearSpectral3D(mesh, np.float64, speed_of_sound=np.full(mesh.ncells, 1500.0), nodal_medium=medium)
    with pytest.raises(ValueError, match="nodal_medium"):
        ls.LinearSpectral3D(mesh, np.float64, density=np.full(mesh.ncells, 1000.0), nodal_medium=medium)
    with pytest.raises(ValueError, match="affine"):
        ls.LinearSpectral3D(_solver_mesh(perturbed=False), np.float64, affine=True, nodal_medium=medium)
    box = ls.LinearSpectral3D(_solver_mesh(perturbed=False), np.float64, nodal_medium=medium)  # an affine box is a trilinear mesh
    assert box.in_kernel_geometry and not box.affine and box.stiff.nodal is not None and box.G_array is None
    low = ls.LinearSpectral3D(pkg("boxmesh").BoxMesh(1, (2, 2, 2), length=0.004), np.float64, nodal_medium=medium)  # below the "auto" degree too
    assert low.in_kernel_geometry and low.stiff.nodal is not None


def test_partitioned_solver_with_nodal_medium(gpu):
    """Two ranks sharing cuda:0 in this process, grid (2, 1, 1), the set-up exchange deferred to the driver: each rank evaluates the lens
    at its own dofs, ghosts included (nothing is exchanged for the medium), the lumped mass takes its nodal factor after the reverse
    exchange, and the cell sub-ranges of the halo schedule pass x -- and with it the operator's coefficient -- whole.  Against the
    single-rank run by lexicographic id over the owned dofs, to 1e-11."""
    import torch

    ls, scat, utils = pkg("linear_solver"), pkg("scatterer"), pkg("utils")
    R, nsteps = 2, 8
    meshes = [_solver_mesh(perturbed=False, grid=(2, 1, 1), rank=r) for r in range(R)]
    serial = _solver_mesh(perturbed=False)
    dt, tf = _time_step(serial)
    one = ls.LinearSpectral3D(serial, np.float64, nodal_medium=_lens_medium())
    one.init()
    one.rk4(0.0, tf, dt, max_steps=nsteps)
    u_one, v_one = one.u_sol(), one.v_sol()
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    solvers = [ls.LinearSpectral3D(meshes[r], np.float64, comm=scat.NativeComm(local=(8400, R, r)), halo_plan=(od[r], gd[r]),
                                   defer_setup_exchange=True, nodal_medium=_lens_medium()) for r in range(R)]
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        assert s.halo is not None and s.stiff.nodal.numel() == s.ndofs
        s.init()
    res = _lockstep([s.rk4_schedule(0.0, tf, dt, max_steps=nsteps) for s in solvers])
    torch.cuda.synchronize()
    assert all(r[1] == nsteps for r in res) and np.max(np.abs(u_one)) > 0
    seen = np.zeros(u_one.size, dtype=int)
    for m, s in zip(meshes, solvers):
        lex = m.global_lexicographic_ids()[: m.nlocal]
        seen[lex] += 1
        du, dv = rel_l2(s.u_sol(), u_one[lex]), rel_l2(s.v_sol(), v_one[lex])
        print(f"rank {m.rank}: rel l2 to the single-rank run u {du:.3e} v {dv:.3e}")
        assert du < 1e-11 and dv < 1e-11
        assert s.halo.health() == 0
    assert np.all(seen == 1)


def _lateral(mesh, c, cells=1):
    """A sponge layer of ``cells`` cells inside the four lateral faces (y and z) of the box (as tests/test_sponge_gpu.py)."""
    sp = pkg("sponge")
    hy, hz = (mesh.length[a] / mesh.global_cells[a] for a in (1, 2))
    return sp.box_profile((0.0, 0.0, 0.0), mesh.length, (mesh.length[0], cells * hy, cells * hz), sp.LATERAL, c)


def test_attachments_with_nodal_medium_match_model(gpu):
    """One run with a sponge layer, two point sources next to the facet source, one relaxation mechanism (scalar weight) and a
    ``PointSensors`` recorder: 12 steps against the CPU loop with the same hooks (tests/sponge_cpu.py, point_source_cpu.py, the loop of
    relaxation_cpu.py) to 1e-11, the recorded series against the model's field at the points after every step."""
    ls, sp, src, rx, sens, pe = (pkg(m) for m in ("linear_solver", "sponge", "sources", "relaxation", "sensors", "point_evaluation"))
    mesh, dt, tf, c, rho, _ = _solver_case()
    steps = 12
    L = np.asarray(mesh.length)
    sigma = _lateral(mesh, _C[0])
    ps = src.PointSources(np.array([[0.41, 0.57, 0.36], [0.68, 0.31, 0.62]]) * L, amplitude=[0.05, 0.03], phase=[0.0, 1.1], delay=[0.0, 2.5 * dt])
    tau, kappa = np.array([8e-7]), np.array([0.05])
    pts = np.array([[0.3, 0.5, 0.5], [0.5, 0.45, 0.6], [0.8, 0.3, 0.4]]) * L
    s = ls.LinearSpectral3D(mesh, np.float64, nodal_medium=_lens_medium(), sponge=sp.SpongeLayer(sigma), point_source=ps,
                            relaxation=rx.RelaxationAbsorption(tau, kappa))
    rec = sens.PointSensors(mesh, pts, np.float64, capacity=steps)
    s.init()
    _, done = s.rk4(0.0, tf, dt, max_steps=steps, sensors=rec)
    assert done == steps and rec.nrec == steps and s._sponge[0].numel() > 0 and s._points.npoints == 2
    fd1 = mesh.facet_dofmap(mesh.boundary_facets([2]))
    rows = []
    u_ref, v_ref, xi_ref = nodal_cpu.solve(
        mesh, steps, dt, c, rho, f0=F0, stage_term=sponge_cpu.layer_term(mesh, sigma),
        source_term=point_source_cpu.point_term(mesh, ps, F0, facet_scale=(60000.0 * 2 * np.pi * F0 / c[fd1].mean(), 4.0)),
        relaxation=(tau, kappa), record=lambda t, u, v: rows.append(pe.eval_function(mesh, u, rec.points, rec.setup.cells)))
    plain = _solver_case()[5][0]
    du, dv = rel_l2(s.u_sol(), u_ref), rel_l2(s.v_sol(), v_ref)
    dx = float(np.linalg.norm(s._relax.xi0[:, : s.nlocal].cpu().numpy() - xi_ref) / np.linalg.norm(u_ref))
    series, rows = rec.series(), np.asarray(rows)
    ds = float(np.max(np.abs(series - rows)) / np.max(np.abs(rows)))
    print(f"attachments: rel l2 to the model u {du:.3e} v {dv:.3e} xi {dx:.3e}; sensor series {ds:.3e}")
    assert np.max(np.abs(u_ref)) > 0 and np.max(np.abs(xi_ref)) > 0 and np.max(np.abs(rows)) > 0 and plain.shape == u_ref.shape
    assert du < 1e-11 and dv < 1e-11 and dx < 1e-11 and ds < 1e-11


def test_graph_replay_with_nodal_medium_matches_rk4(gpu):
    """rk4_graph replays a plain nodal step: the operator's coefficient is a fixed device pointer, captured with the launch -- the
    replayed steps (and the shorter last one through rk4) equal rk4's at the existing replay bar (1e-13)."""
    ls = pkg("linear_solver")
    mesh, dt, _, _, _, _ = _solver_case()
    tf = 14.5 * dt  # 14 full steps and a shorter last one
    a, b = (ls.LinearSpectral3D(mesh, np.float64, nodal_medium=_lens_medium()) for _ in range(2))
    for s in (a, b):
        s.init()
    ta, sa = a.rk4(0.0, tf, dt)
    t1, s1 = b.rk4_graph(0.0, tf, dt, max_steps=6)  # captures
    t2, s2 = b.rk4_graph(t1, tf, dt)  # replays the same graph, then the short last step
    assert sa == 15 and s1 == 6 and s1 + s2 == sa and abs(t2 - ta) < 1e-18 and len(b._graphs) == 1
    assert np.max(np.abs(a.u_sol())) > 0
    du, dv = rel_l2(b.u_sol(), a.u_sol()), rel_l2(b.v_sol(), a.v_sol())
    print(f"graph replay against rk4: u {du:.3e} v {dv:.3e}")
    assert du < 1e-13 and dv < 1e-13
