"""The Westervelt solver with a nodal medium on the GPU: the fused cell pass with two nodal coefficients and the geometry formed in the
kernel (csrc/westervelt_geom_nodal.hpp) against the CPU model (tests/westervelt_nodal_cpu.py: the oracle's apply on the two pre-scaled
G arrays), its plan shapes and its identities with the existing kernels; ``WesterveltSpectral3D(nodal_medium=...)`` -- the fused stage,
the reference launch sequence and the two-launch cell pass -- against the CPU loop, partitioned, with the attachments, and replayed
from a hipGraph.  Shapes are those of tests/test_nodal_gpu.py."""

import numpy as np
import pytest

import nodal_cpu
import point_source_cpu
import sponge_cpu
import westervelt_nodal_cpu
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
    """A perturbed (non-affine) box; kappa3 and kappa4 two DIFFERENT smooth positive fields with a 3 : 1 range each (a swap is caught);
    c3, c4 different random per-cell constants; u, v independent; and the CPU model's ``b0 + K(c3 kappa3) u + K(c4 kappa4) v`` on a
    non-zero b0 -- computed once per case, read-only."""
    key = (P, cells, np.dtype(dtype).name)
    if key not in _problems:
        pb = build_problem(P, cells, dtype=dtype, perturb=0.2, seed=40 + P)
        mesh = pb["mesh"]
        xyz = mesh.dof_coordinates()
        k3 = nodal_cpu.smooth_field(xyz, 1.0, 3.0, 1.0).astype(dtype)
        k4 = nodal_cpu.smooth_field(xyz[:, ::-1] + 0.35, 0.5, 1.5, 1.0).astype(dtype)
        for k in (k3, k4):
            assert k.min() > 0 and k.max() / k.min() > 2.5
        assert rel_l2(k3, k4) > 0.3
        rng = np.random.default_rng(100 + P)
        v = rng.standard_normal(mesh.ndofs).astype(dtype) * np.abs(pb["x"]).max().astype(dtype)
        c4 = (0.5 + rng.random(mesh.ncells)).astype(dtype)
        b0 = (rng.standard_normal(mesh.ndofs) * 10.0).astype(dtype)
        b_ref = b0.astype(np.float64)
        westervelt_nodal_cpu.stiffness_pair(P, pb["D"].astype(np.float64), pb["x"].astype(np.float64), v.astype(np.float64),
                                            pb["cc"].astype(np.float64), c4.astype(np.float64), b_ref, pb["G"].astype(np.float64),
                                            mesh.dofmap, k3.astype(np.float64), k4.astype(np.float64))
        for a in (b0, b_ref, k3, k4, v, c4):
            a.setflags(write=False)
        pb.update(k3=k3, k4=k4, v=v, c4=c4, b0=b0, b_ref=b_ref)
        _problems[key] = pb
    return _problems[key]


def _geometry(pb, x_dofs=None):
    mesh = pb["mesh"]
    return (mesh.x_dofs if x_dofs is None else x_dofs, mesh.x_g, pb["pts"], pb["wts"])


def _pair_operator(ops, pb, dtype, nodal=None):
    return ops.westervelt_cell_operator(pb["P"], pb["D"].flatten(), dtype, geometry=_geometry(pb)[1:],
                                        nodal=(pb["k3"], pb["k4"]) if nodal is None else nodal)


def _apply(dev, op, pb, u=None, v=None, c3=None, c4=None, b0=None, dofmap=None, x_dofs=None):
    mesh = pb["mesh"]
    pick = lambda a, default: default if a is None else a  # noqa: E731
    b = dev.to_device(np.ascontiguousarray(pick(b0, np.zeros(mesh.ndofs, dtype=pb["x"].dtype))).copy())
    op.stiffness_only(dev.to_device(np.ascontiguousarray(pick(u, pb["x"]))), dev.to_device(np.ascontiguousarray(pick(v, pb["v"]))),
                      dev.to_device(pick(c3, pb["cc"])), dev.to_device(pick(c4, pb["c4"])), b,
                      dev.to_device(pick(x_dofs, mesh.x_dofs)), dev.to_device(pick(dofmap, mesh.dofmap)))
    return b.copy_to_host()


_CASES = [(P, (3, 2, 2), np.float64) for P in range(1, 11)] + [(2, (4, 3, 3), np.float64)] + [(P, (3, 2, 2), np.float32) for P in (2, 4, 6)]


@pytest.mark.parametrize("P,cells,dtype", _CASES, ids=[f"P{P}-{'x'.join(map(str, c))}-{np.dtype(d).name}" for P, c, d in _CASES])
def test_operator_matches_cpu_model(gpu, P, cells, dtype):
    """b += K(c3 kappa3) u + K(c4 kappa4) v on top of a non-zero b, against the oracle's applies on G kappa[dofmap]: every degree on
    3 x 2 x 2 cells (fp64), P = 2 on 36 cells (more than one batch of 28, with a tail), fp32 at P = 2, 4, 6."""
    dev, ops = gpu
    pb = _problem(P, cells, dtype)
    op = _pair_operator(ops, pb, dtype)
    assert all(k.numel() == pb["mesh"].ndofs and k.is_cuda for k in op.nodal)
    b = _apply(dev, op, pb, b0=pb["b0"])
    _check(b, pb["b_ref"], dtype, f"nodal Westervelt cell pass P={P} {cells} {np.dtype(dtype).name}")
    assert rel_l2(b, pb["b0"]) > 1e-2  # the apply added something


def test_plan_shapes(gpu):
    """P = 4, 24 cells: the same apply through an ordered plan (rows of the dofmap, of x_dofs and the constants permuted at random) and
    with FUS_TUNE_PLAN_RUNS both ways -- all four (ORDERED, RUNS) builds -- equals the plain one to 1e-12."""
    dev, ops = gpu
    lib = pkg("_lib")
    pb = _problem(4, (4, 3, 2))
    mesh = pb["mesh"]
    op = _pair_operator(ops, pb, np.float64)
    perm = np.random.default_rng(3).permutation(mesh.ncells)
    permuted = tuple(np.ascontiguousarray(a[perm]) for a in (mesh.dofmap, mesh.x_dofs, pb["cc"], pb["c4"]))
    natural = (mesh.dofmap, mesh.x_dofs, pb["cc"], pb["c4"])
    apply = lambda dm, xd, c3, c4: _apply(dev, op, pb, c3=c3, c4=c4, dofmap=dm, x_dofs=xd)  # noqa: E731
    ops._PLANS.clear()
    try:
        plain = apply(*natural)
        assert ops._PLANS.last_order is None
        _check(plain, pb["b_ref"] - pb["b0"], np.float64, "plain")
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


@pytest.mark.parametrize("P,cells", [(2, (4, 3, 3)), (4, (4, 3, 2)), (5, (3, 2, 2)), (6, (3, 2, 2))], ids=["P2", "P4", "P5", "P6"])
def test_identities_with_the_existing_kernels(gpu, P, cells):
    """Each within TOL: the pass equals two launches of the existing nodal stiffness operator; with v = 0 it is the nodal kernel on u;
    with constant kappa it is ``westervelt_cell_operator(geometry=).stiffness_only`` with per-cell constants; it is linear in (u, v)."""
    dev, ops = gpu
    pb = _problem(P, cells)
    mesh = pb["mesh"]
    Df, dm = pb["D"].flatten(), dev.to_device(mesh.dofmap)
    op = _pair_operator(ops, pb, np.float64)
    got = _apply(dev, op, pb)

    def nodal_launch(x, cc, kappa, y):
        ops.stiffness_operator(P, Df, np.float64, geometry=_geometry(pb), nodal=kappa)(dev.to_device(np.ascontiguousarray(x)), dev.to_device(cc), y, None, dm)

    y = dev.to_device(np.zeros(mesh.ndofs))
    nodal_launch(pb["x"], pb["cc"], pb["k3"], y)
    only_u = y.copy_to_host()
    nodal_launch(pb["v"], pb["c4"], pb["k4"], y)
    _check(got, y.copy_to_host(), np.float64, f"P={P}: against two launches of the nodal operator")
    _check(_apply(dev, op, pb, v=np.zeros(mesh.ndofs)), only_u, np.float64, f"P={P}: v = 0 against the nodal kernel on u")
    const = _pair_operator(ops, pb, np.float64, nodal=(np.full(mesh.ndofs, 2.5), np.full(mesh.ndofs, 0.75)))
    percell = ops.westervelt_cell_operator(P, Df, np.float64, geometry=_geometry(pb)[1:])
    ref = _apply(dev, percell, pb, c3=2.5 * pb["cc"], c4=0.75 * pb["c4"])
    assert np.max(np.abs(ref)) > 0
    _check(_apply(dev, const, pb), ref, np.float64, f"P={P}: constant kappa against the per-cell two-gather pass")
    rng = np.random.default_rng(9)
    u2, v2 = rng.standard_normal(mesh.ndofs) * 50.0, rng.standard_normal(mesh.ndofs) * 50.0
    combined = _apply(dev, op, pb, u=2.0 * pb["x"] - 3.0 * u2, v=2.0 * pb["v"] - 3.0 * v2)
    _check(combined, 2.0 * got - 3.0 * _apply(dev, op, pb, u=u2, v=v2), np.float64, f"P={P}: linearity in (u, v)")


def test_operator_argument_checks(gpu):
    dev, ops = gpu
    pb = _problem(2, (3, 2, 2))
    mesh = pb["mesh"]
    Df = pb["D"].flatten()
    t = dev.to_device
    u, v, c3, c4, dm, xd = t(pb["x"]), t(pb["v"]), t(pb["cc"]), t(pb["c4"]), t(mesh.dofmap), t(mesh.x_dofs)
    b = t(np.zeros(mesh.ndofs))
    with pytest.raises(ValueError, match="needs geometry"):
        ops.westervelt_cell_operator(2, Df, np.float64, nodal=(pb["k3"], pb["k4"]))
    with pytest.raises(ValueError, match="one value per dof"):
        _pair_operator(ops, pb, np.float64, nodal=(pb["k3"][:-1], pb["k4"][:-1])).stiffness_only(u, v, c3, c4, b, xd, dm)
    with pytest.raises(ValueError, match="differ in length"):
        _pair_operator(ops, pb, np.float64, nodal=(pb["k3"], pb["k4"][:-1]))
    with pytest.raises(ValueError, match="two coefficient vectors"):
        _pair_operator(ops, pb, np.float64, nodal=(pb["k3"],))
    op = _pair_operator(ops, pb, np.float64)
    with pytest.raises(ValueError, match="no mass part"):
        op(u, v, c3, c3, c4, c4, b, t(np.zeros(mesh.ndofs)), xd, dm)
    with pytest.raises(ValueError, match="one value per cell"):
        op.stiffness_only(u, v, c3[:-1], c4, b, xd, dm)
    with pytest.raises(ValueError, match="x_dofs"):
        op.stiffness_only(u, v, c3, c4, b, xd[:-1], dm)
    op32 = _pair_operator(ops, pb, np.float32)  # the coefficients take the operator's type
    assert all(k.dtype == pkg("_lib").torch_dtype(np.float32) for k in op32.nodal)
    with pytest.raises(TypeError):
        op32.stiffness_only(u, v, c3, c4, b, xd, dm)
    op.stiffness_only(u, v, c3[:0], c4[:0], b, xd[:0], dm[:0])  # an empty cell range: nothing is launched
    assert not np.any(b.copy_to_host())


# ---- the solver --------------------------------------------------------------------------------------------------------------------
_P, _CELLS, _L, _STEPS = 3, (4, 2, 2), (0.012, 0.006, 0.006), 20
_C, _RHO, _BETA, _ATT = (1500.0, 2400.0), (1000.0, 1800.0), (3.5, 6.0), (0.2, 8.0)  # water, and the peak of the inclusion
_P0 = 1.0e6  # source amplitude [Pa]: chosen on the CPU model so that halving beta moves u by far more than 100 x the parity bar
_BAR = 1e-11  # the bar of tests/test_nodal_gpu.py and of the existing Westervelt solver tests (test_solver_gpu.py, test_sponge_gpu.py, ...)
_cache = {}


def _lens_medium(length=_L, beta_scale=1.0):
    """A smooth Gaussian inclusion in c, rho, beta and alpha at the middle of the box (its tail reaches the source and absorbing faces)."""
    center, radius = 0.5 * np.asarray(length), 0.3 * length[1]
    beta = nodal_cpu.lens(center, radius, *_BETA)
    return pkg("nodal_medium").NodalMedium(nodal_cpu.lens(center, radius, *_C), nodal_cpu.lens(center, radius, *_RHO),
                                           nonlinear_coefficient=lambda xyz: beta_scale * beta(xyz),
                                           attenuation_coefficient_dB=nodal_cpu.lens(center, radius, *_ATT))


def _solver_mesh(perturbed=True, **kw):
    return pkg("boxmesh").BoxMesh(_P, _CELLS, length=_L, **(dict(perturb=0.1, seed=7) if perturbed else {}), **kw)


def _time_step(mesh):
    ls = pkg("linear_solver")
    h = ls.time_step_parameters(mesh, _P, _C[1], F0, mesh.length[0])
    dt, _, _ = ls.snap_time_step(h, _P, _C[1], F0, mesh.length[0])  # the fastest speed of the medium bounds the step
    return dt, 1000 * dt  # a final time no run here reaches: max_steps ends them


def _solver(mesh, medium=None, **kw):
    kw.setdefault("fused", True)
    kw.setdefault("source_amplitude", _P0)
    return pkg("nonlinear_solver").WesterveltSpectral3D(mesh, np.float64, source_frequency=F0,
                                                        nodal_medium=_lens_medium() if medium is None else medium, **kw)


def _solver_case():
    if "plain" not in _cache:
        mesh = _solver_mesh()
        dt, tf = _time_step(mesh)
        fields = _lens_medium().evaluate_westervelt(mesh)
        c, rho, beta, att = fields
        assert c.max() / c.min() > 1.4 and rho.max() / rho.min() > 1.5 and beta.max() / beta.min() > 1.5 and att.max() / att.min() > 10
        ref = westervelt_nodal_cpu.solve(mesh, _STEPS, dt, *fields, f0=F0, p0=_P0)
        half = westervelt_nodal_cpu.solve(mesh, _STEPS, dt, c, rho, 0.5 * beta, att, f0=F0, p0=_P0)
        for a in ref + half:
            a.setflags(write=False)
        _cache["plain"] = (mesh, dt, tf, fields, ref, half)
    return _cache["plain"]


@pytest.mark.parametrize("variant", ["fused", "reference-sequence", "two-launch"])
def test_solver_with_nodal_medium_matches_model(gpu, variant):
    """20 steps at P = 3 on a perturbed 4 x 2 x 2 box with a smooth lens in all four fields: the fused stage with the new cell pass,
    the reference launch sequence (two launches of the nodal stiffness operator, pointwise products with w2 / w5) and the fused stage
    with ``nodal_cell_pass="two-launch"``, each against the CPU loop to 1e-11.  The lens is not a no-op, and the amplitude is such
    that halving beta moves u by more than 100 x the bar: the nonlinear diagonals are exercised."""
    mesh, dt, tf, (c, rho, beta, att), (u_ref, v_ref), (u_half, _) = _solver_case()
    kw = dict(fused=False) if variant == "reference-sequence" else dict(nodal_cell_pass="two-launch" if variant == "two-launch" else "fused")
    s = _solver(mesh, **kw)
    assert s.in_kernel_geometry and s.kappa is None and s.nodal_cell_pass == ("two-launch" if variant == "two-launch" else "fused")
    assert all(np.array_equal(a, b) for a, b in zip((s.c_nodal, s.rho_nodal, s.beta_nodal, s.att_nodal), (c, rho, beta, att)))
    means = lambda a: a[mesh.dofmap].mean(axis=1)  # noqa: E731
    delta = westervelt_nodal_cpu.diffusivity(2 * np.pi * F0, c, att)
    assert np.allclose(s.c_cells, means(c)) and np.allclose(s.rho_cells, means(rho)) and np.allclose(s.delta_cells, means(delta), rtol=1e-12)
    fd1 = mesh.facet_dofmap(mesh.boundary_facets([2]))
    assert abs(s.c0 - c[fd1].mean()) < 1e-9 and abs(s.rho0 - rho[fd1].mean()) < 1e-9
    assert abs(s.beta - means(beta).mean()) < 1e-12 and abs(s.delta - means(delta).mean()) < 1e-12 * s.delta
    s.init()
    _, steps = s.rk4(0.0, tf, dt, max_steps=_STEPS)
    assert steps == _STEPS
    u, v = s.u_sol(), s.v_sol()
    du, dv = rel_l2(u, u_ref), rel_l2(v, v_ref)
    if "water" not in _cache:
        w = pkg("nonlinear_solver").WesterveltSpectral3D(mesh, np.float64, speed_of_sound=_C[0], density=_RHO[0], nonlinear_coefficient=_BETA[0],
                                                         attenuation_coefficient_dB=_ATT[0], source_frequency=F0, source_amplitude=_P0, fused=True)
        w.init()
        w.rk4(0.0, tf, dt, max_steps=_STEPS)
        _cache["water"] = w.u_sol()
    nonlinear = rel_l2(u_half, u_ref)
    print(f"{variant}: rel l2 to the model u {du:.3e} v {dv:.3e}; to the homogeneous solver u {rel_l2(u, _cache['water']):.3e}; "
          f"halving beta moves the model's u by {nonlinear:.3e}")
    assert np.max(np.abs(u_ref)) > 0
    assert nonlinear > 100 * _BAR
    assert du < _BAR and dv < _BAR
    assert rel_l2(u, _cache["water"]) > 1e-3


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
def test_constant_nodal_values_equal_the_scalar_medium(gpu, fused):
    """Constant nodal values -- scalars, constant arrays, constant callables -- against the scalar-medium solver with
    ``in_kernel_geometry=True`` to 1e-12: stiffness, the three diagonals, facet means and the reference scalars reduce to the scalar forms."""
    nls, nm = pkg("nonlinear_solver"), pkg("nodal_medium")
    mesh = _solver_mesh()
    dt, tf = _time_step(mesh)
    vals = dict(speed_of_sound=1540.0, density=1050.0, nonlinear_coefficient=4.2, attenuation_coefficient_dB=0.7)
    kw = dict(source_frequency=F0, source_amplitude=_P0, fused=fused)
    ref = nls.WesterveltSpectral3D(mesh, np.float64, in_kernel_geometry=True, **vals, **kw)
    full = lambda a: np.full(mesh.ndofs, a)  # noqa: E731
    call = lambda a: (lambda xyz: np.full(xyz.shape[0], a))  # noqa: E731
    media = (nm.NodalMedium(1540.0, 1050.0, nonlinear_coefficient=4.2, attenuation_coefficient_dB=0.7),
             nm.NodalMedium(full(1540.0), full(1050.0), nonlinear_coefficient=full(4.2), attenuation_coefficient_dB=full(0.7)),
             nm.NodalMedium(call(1540.0), call(1050.0), nonlinear_coefficient=call(4.2), attenuation_coefficient_dB=call(0.7)))
    runs = [ref] + [nls.WesterveltSpectral3D(mesh, np.float64, nodal_medium=m, **kw) for m in media]
    # ... and a field the medium leaves None takes the solver's scalar
    runs.append(nls.WesterveltSpectral3D(mesh, np.float64, nodal_medium=nm.NodalMedium(1540.0, 1050.0), nonlinear_coefficient=4.2,
                                         attenuation_coefficient_dB=0.7, **kw))
    for s in runs:
        s.init()
        s.rk4(0.0, tf, dt, max_steps=_STEPS)
    assert np.max(np.abs(ref.u_sol())) > 0 and abs(runs[1].c0 - 1540.0) < 1e-9 and abs(runs[1].rho0 - 1050.0) < 1e-9
    for s in runs[1:]:
        du, dv = rel_l2(s.u_sol(), ref.u_sol()), rel_l2(s.v_sol(), ref.v_sol())
        print(f"constant nodal medium against the scalar medium: u {du:.3e} v {dv:.3e}")
        assert du < 1e-12 and dv < 1e-12


def test_solver_argument_conflicts(gpu):
    nls, nm = pkg("nonlinear_solver"), pkg("nodal_medium")
    mesh = _solver_mesh()
    medium = nm.NodalMedium(1500.0, 1000.0)
    per_cell = np.full(mesh.ncells, 1.0)
    for name, value in (("speed_of_sound", 1500.0), ("density", 1000.0), ("nonlinear_coefficient", 3.5), ("attenuation_coefficient_dB", 0.2)):
        with pytest.raises(ValueError, match=f"nodal_medium.*{name}"):
            nls.WesterveltSpectral3D(mesh, np.float64, nodal_medium=medium, **{name: value * per_cell})
    with pytest.raises(ValueError, match="uniform_ratio"):
        nls.WesterveltSpectral3D(mesh, np.float64, nodal_medium=medium, uniform_ratio=True)
    with pytest.raises(ValueError, match="in_kernel_geometry=False.*not worth carrying"):
        nls.WesterveltSpectral3D(mesh, np.float64, nodal_medium=medium, in_kernel_geometry=False)
    with pytest.raises(ValueError, match="nodal_cell_pass"):
        nls.WesterveltSpectral3D(mesh, np.float64, nodal_medium=medium, nodal_cell_pass="three-launch")
    # in-kernel geometry at every degree and in both stage implementations, on an affine box too
    for fused in (True, False):
        low = nls.WesterveltSpectral3D(pkg("boxmesh").BoxMesh(1, (2, 2, 2), length=0.004), np.float64, nodal_medium=medium, fused=fused)
        assert low.in_kernel_geometry and low.cell_nodal.nodal[0].numel() == low.ndofs
    plain = nls.WesterveltSpectral3D(mesh, np.float64, fused=True)  # without the keyword nothing is new
    assert plain.nodal_medium is None and plain.nodal_cell_pass is None and not hasattr(plain, "cell_nodal")


def test_partitioned_solver_with_nodal_medium(gpu):
    """Two ranks sharing cuda:0 in this process, grid (2, 1, 1), the set-up exchange deferred to the driver: each rank evaluates the lens
    at its own dofs, ghosts included (nothing is exchanged for the medium), the three diagonals take their nodal factors before the one
    grouped reverse exchange, and the cell sub-ranges of the halo schedule pass u and v -- and with them the operator's coefficients --
    whole.  Against the single-rank run by lexicographic id over the owned dofs, to 1e-11."""
    import torch

    scat, utils = pkg("scatterer"), pkg("utils")
    R, nsteps = 2, 8
    meshes = [_solver_mesh(perturbed=False, grid=(2, 1, 1), rank=r) for r in range(R)]
    serial = _solver_mesh(perturbed=False)
    dt, tf = _time_step(serial)
    one = _solver(serial)
    one.init()
    one.rk4(0.0, tf, dt, max_steps=nsteps)
    u_one, v_one = one.u_sol(), one.v_sol()
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    solvers = [_solver(meshes[r], comm=scat.NativeComm(local=(8410, R, r)), halo_plan=(od[r], gd[r]), defer_setup_exchange=True)
               for r in range(R)]
    _lockstep([s._setup for s in solvers])
    for s in solvers:
        assert s.halo is not None and s.cell_nodal.nodal[0].numel() == s.ndofs
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
    """One run with a sponge layer, two point sources (the facet source silenced) and one relaxation mechanism (scalar weight): 12 steps
    against the CPU loop with the same hooks (tests/sponge_cpu.py, point_source_cpu.py, the loop of relaxation_cpu.py) to 1e-11."""
    sp, src, rx = (pkg(m) for m in ("sponge", "sources", "relaxation"))
    mesh, dt, tf, fields, _, _ = _solver_case()
    steps = 12
    L = np.asarray(mesh.length)
    sigma = _lateral(mesh, _C[0])
    ps = src.PointSources(np.array([[0.41, 0.57, 0.36], [0.68, 0.31, 0.62]]) * L, amplitude=[0.05, 0.03], phase=[0.0, 1.1], delay=[0.0, 2.5 * dt])
    tau, kappa = np.array([8e-7]), np.array([0.05])
    s = _solver(mesh, sponge=sp.SpongeLayer(sigma), point_source=ps, relaxation=rx.RelaxationAbsorption(tau, kappa), source_amplitude=0.0)
    s.init()
    _, done = s.rk4(0.0, tf, dt, max_steps=steps)
    assert done == steps and s._sponge[0].numel() > 0 and s._points.npoints == 2
    u_ref, v_ref, xi_ref = westervelt_nodal_cpu.solve(mesh, steps, dt, *fields, f0=F0, p0=0.0, stage_term=sponge_cpu.layer_term(mesh, sigma),
                                                      source_term=point_source_cpu.point_term(mesh, ps, F0), relaxation=(tau, kappa))
    du, dv = rel_l2(s.u_sol(), u_ref), rel_l2(s.v_sol(), v_ref)
    dx = float(np.linalg.norm(s._relax.xi0[:, : s.nlocal].cpu().numpy() - xi_ref) / np.linalg.norm(u_ref))
    print(f"attachments: rel l2 to the model u {du:.3e} v {dv:.3e} xi {dx:.3e}")
    assert np.max(np.abs(u_ref)) > 0 and np.max(np.abs(xi_ref)) > 0
    assert du < 1e-11 and dv < 1e-11 and dx < 1e-11


def test_graph_replay_with_nodal_medium_matches_rk4(gpu):
    """rk4_graph replays a nodal step: the operator's coefficients are fixed device pointers, captured with the launch -- the replayed
    steps (and the shorter last one through rk4) equal rk4's at the existing replay bar (1e-13)."""
    mesh, dt, _, _, _, _ = _solver_case()
    tf = 14.5 * dt  # 14 full steps and a shorter last one
    a, b = (_solver(mesh) for _ in range(2))
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
