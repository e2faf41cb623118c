"""Absorbing sponge layers on the GPU: the sparse kernel (csrc/sponge.hpp) against numpy, both wave solvers with a layer -- every stage
implementation -- against the CPU model (oracle/rk4_oracle.py with the stage term of tests/sponge_cpu.py), the empty
layer, hipGraph replay, partitioned runs and fp32."""

import numpy as np
import pytest

import sponge_cpu
from conftest import TOL, pkg, rel_l2, rel_max
from oracle import rk4_oracle

pytestmark = pytest.mark.gpu

_lockstep = pkg("solver_base").run_lockstep


def _lateral(mesh, c, cells=1):
    """A layer of ``cells`` cells inside the four lateral faces (y and z) of the mesh's global box."""
    sp = pkg("sponge")
    hy, hz = (mesh.length[a] / mesh.global_cells[a] for a in (1, 2))
    return sp.box_profile((0.0, 0.0, 0.0), mesh.length, (mesh.length[0], cells * hy, cells * hz), sp.LATERAL, c)


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("n", [0, 1, 257, 1000])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_sponge_terms_kernel(dtype, n, offset):
    """y[idx] -= cv v[idx] + cu u[idx] on a y filled with nonzero values; operands 256-byte aligned, and every one of them one element
    further; the entries of y outside the list keep their bits."""
    _sponge_case(dtype, n, offset)


def _sponge_case(dtype, n, offset, nd=3000, idx=None, figures=None):
    """The launch of ``test_sponge_terms_kernel`` and its checks on a vector of ``nd`` entries; ``idx``: the list (ascending, distinct;
    default: the test's own for ``n``).  Returns y as the launch left it."""
    import torch

    torch.cuda.set_device(0)
    ops = pkg("operators")
    rng = np.random.default_rng(100 * n + offset)
    if idx is not None:
        assert idx.dtype == np.int32 and idx.size == n and np.all(np.diff(idx) > 0) and idx[-1] < nd
    elif n == 1000:  # gaps: 1000 of 3000, runs and holes of every small length
        idx = np.sort(rng.choice(nd, size=n, replace=False)).astype(np.int32)
        assert np.any(np.diff(idx) > 1) and np.any(np.diff(idx) == 1)
    else:  # one run: more than one workgroup at 257
        idx = (np.arange(n) + 41).astype(np.int32)
    y, u, v = (rng.uniform(0.5, 2.0, nd).astype(dtype) * rng.choice([-1.0, 1.0], nd).astype(dtype) for _ in range(3))
    cu, cv = rng.uniform(0.1, 1.0, n).astype(dtype), rng.uniform(0.1, 1.0, n).astype(dtype)

    def dev(a):  # the array at an element offset into its own allocation (allocations are 256-byte aligned)
        buf = torch.zeros(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
        view = buf[offset:]
        view.copy_(torch.from_numpy(a))
        assert a.size == 0 or view.data_ptr() % 256 == offset * a.itemsize  # (an empty tensor has no address)
        return view

    y_d, u_d, v_d, idx_d, cu_d, cv_d = (dev(a) for a in (y, u, v, idx, cu, cv))
    ops.sponge_terms(y_d, u_d, v_d, (idx_d, cu_d, cv_d))
    torch.cuda.synchronize()
    got = y_d.cpu().numpy()
    ref = y.astype(np.float64)
    ref[idx] -= cv.astype(np.float64) * v.astype(np.float64)[idx] + cu.astype(np.float64) * u.astype(np.float64)[idx]
    tol = TOL[np.dtype(dtype)]
    assert rel_l2(got, ref) < tol["l2"] and rel_max(got, ref) < tol["mx"]
    if n:
        # on the list alone, against the size of the three terms (each at most 2: a difference may cancel, the bound may not)
        assert np.max(np.abs(got[idx] - ref[idx])) < tol["mx"] * 6.0 and not np.any(got[idx] == y[idx])
    outside = np.ones(nd, dtype=bool)
    outside[idx] = False
    assert np.array_equal(got[outside].view(np.uint8), y[outside].view(np.uint8))
    if figures is not None and n:
        figures["list"] = float(np.max(np.abs(got[idx] - ref[idx])) / (tol["mx"] * 6.0))
    return got


def test_sponge_terms_argument_checks():
    import torch

    torch.cuda.set_device(0)
    ops, lib_mod = pkg("operators"), pkg("_lib")
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        ops.sponge_terms(z(8), z(8), z(8, torch.float32), (idx, z(4), z(4)))
    with pytest.raises(TypeError):
        ops.sponge_terms(z(8), z(8), z(8), (idx.long(), z(4), z(4)))
    with pytest.raises(ValueError):
        ops.sponge_terms(z(8), z(8), z(8), (idx, z(4), z(3)))
    with pytest.raises(ValueError):
        ops.sponge_terms(z(8), z(7), z(8), (idx, z(4), z(4)))
    with pytest.raises(lib_mod.FusGpuError):
        ops.sponge_terms(z(8), z(8), z(8).cpu(), (idx, z(4), z(4)))  # no CPU path


# ---- the linear solver -------------------------------------------------------------------------------------------------------------
_LINEAR = {"box": dict(P=4, cells=(6, 3, 3), length=(0.012, 0.006, 0.006), mesh_kw={}, solver_kw={}, steps=12),
           "perturbed-in-kernel-geometry": dict(P=3, cells=(5, 4, 4), length=0.01, mesh_kw=dict(perturb=0.1, seed=2),
                                                solver_kw=dict(in_kernel_geometry=True), steps=12)}
_model_cache = {}


def _linear_case(name, oracle_c):
    """Mesh, time step, the layer and -- computed once per case -- the model's fields with and without it."""
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    if name not in _model_cache:
        k = _LINEAR[name]
        mesh = boxmesh.BoxMesh(k["P"], k["cells"], length=k["length"], **k["mesh_kw"])
        h = ls.time_step_parameters(mesh, k["P"], 1500.0, 0.5e6, mesh.length[0])
        dt, tf, _ = ls.snap_time_step(h, k["P"], 1500.0, 0.5e6, mesh.length[0])
        sigma = _lateral(mesh, 1500.0)
        with_layer = rk4_oracle.solve(mesh, k["steps"], dt, stage_term=sponge_cpu.layer_term(mesh, sigma), oracle_c=oracle_c)
        without = rk4_oracle.solve(mesh, k["steps"], dt, oracle_c=oracle_c)
        for a in with_layer + without:
            a.setflags(write=False)
        _model_cache[name] = (mesh, dt, tf, sigma, with_layer, without)
    return _model_cache[name]


@pytest.mark.parametrize("variant", ["fused-lean", "fused-reference-kinds", "reference-sequence"])
@pytest.mark.parametrize("case", list(_LINEAR))
def test_linear_solver_with_layer_matches_model(oracle_c, case, variant):
    """One cell of layer inside the y and z faces, 12 steps: the fused stage with the lean vector pass, with the reference's stage kinds
    (lean_stages = False) and the reference launch sequence, each against the CPU model at the bar of tests/test_solver_gpu.py; and the
    layer is not a no-op (the model's fields with and without it differ by about 0.5)."""
    import torch

    torch.cuda.set_device(0)
    ls, sp = pkg("linear_solver"), pkg("sponge")
    mesh, dt, tf, sigma, (u_ref, v_ref), (u_free, v_free) = _linear_case(case, oracle_c)
    k = _LINEAR[case]
    s = ls.LinearSpectral3D(mesh, np.float64, fused=variant != "reference-sequence", sponge=sp.SpongeLayer(sigma), **k["solver_kw"])
    if k["solver_kw"]:
        assert s.in_kernel_geometry
    if variant == "fused-reference-kinds":
        s.lean_stages = False
    assert s.lean_stages == (variant != "fused-reference-kinds") and s._sponge[0].numel() > 0
    s.init()
    _, steps = s.rk4(0.0, tf, dt, max_steps=k["steps"])
    assert steps == k["steps"]
    u, v = s.u_sol(), s.v_sol()
    du, dv = rel_l2(u, u_ref), rel_l2(v, v_ref)
    print(f"{case} {variant}: rel l2 to the model u {du:.3e} v {dv:.3e}; to the layer-free model u {rel_l2(u, u_free):.3e}")
    assert np.max(np.abs(u_ref)) > 0
    assert du < 1e-11 and dv < 1e-11
    assert rel_l2(u, u_free) > 1e-3 and rel_l2(v, v_free) > 1e-3


# ---- the Westervelt solver ---------------------------------------------------------------------------------------------------------
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
        sigma = _lateral(mesh, 1480.0)
        with_layer = rk4_oracle.solve_westervelt(mesh, steps, dt, stage_term=sponge_cpu.layer_term(mesh, sigma), oracle_c=oracle_c)
        without = rk4_oracle.solve_westervelt(mesh, steps, dt, oracle_c=oracle_c)
        for a in with_layer + without:
            a.setflags(write=False)
        _model_cache["westervelt"] = (mesh, dt, tf, steps, sigma, with_layer, without)
    return _model_cache["westervelt"]


@pytest.mark.parametrize("variant", ["fused-two-gather", "fused-uniform-ratio", "reference-sequence"])
def test_westervelt_solver_with_layer_matches_model(oracle_c, variant):
    """Bowl-warped cells, 10 steps, one cell of layer inside the y and z faces, coefficients on m0: the fused stage with the two-gather
    and the single-gather cell pass and the reference launch sequence, each against the CPU model."""
    import torch

    torch.cuda.set_device(0)
    nls, sp = pkg("nonlinear_solver"), pkg("sponge")
    mesh, dt, tf, steps, sigma, (u_ref, v_ref), (u_free, v_free) = _westervelt_case(oracle_c)
    s = nls.WesterveltSpectral3D(mesh, np.float64, fused=variant != "reference-sequence", uniform_ratio=variant == "fused-uniform-ratio",
                                 sponge=sp.SpongeLayer(sigma))
    assert (s.kappa is not None) == (variant == "fused-uniform-ratio")
    s.init()
    _, done = s.rk4(0.0, tf, dt, max_steps=steps)
    assert done == steps
    u, v = s.u_sol(), s.v_sol()
    du, dv = rel_l2(u, u_ref), rel_l2(v, v_ref)
    print(f"westervelt {variant}: rel l2 to the model u {du:.3e} v {dv:.3e}; to the layer-free model u {rel_l2(u, u_free):.3e}")
    assert np.max(np.abs(u_ref)) > 0
    assert du < 1e-11 and dv < 1e-11
    assert rel_l2(u, u_free) > 1e-3


# ---- the empty layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["linear-fused", "linear-reference-sequence", "westervelt-fused"])
def test_empty_layer_changes_nothing(which):
    """sigma == 0 everywhere: the list is empty, no launch is added, and the fields equal those of ``sponge=None`` bit for bit.
    The mesh is a row of cells, 40 x 1 x 1 (two batches of the cell kernels): two runs of the SAME launches differ in the last bits
    wherever a sum of three or more float-atomic adds depends on their order (on a 3 x 3 x 3 box they do, by a few ulp), and on a row
    no entry of b receives more than two addends onto its zero -- two cells, or one cell and one facet -- so every sum is the same in
    either order and the comparison is about the layer alone."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, nls, sp = pkg("boxmesh"), pkg("linear_solver"), pkg("nonlinear_solver"), pkg("sponge")
    mesh = boxmesh.BoxMesh(2, (40, 1, 1), length=(0.04, 0.001, 0.001), perturb=0.1, seed=3)
    h = ls.time_step_parameters(mesh, 2, 1500.0, 0.5e6, 0.04)
    dt, tf, _ = ls.snap_time_step(h, 2, 1500.0, 0.5e6, 0.04)
    res = []
    for layer in (None, sp.SpongeLayer(np.zeros(mesh.nlocal)), sp.SpongeLayer(lambda xyz: np.zeros(xyz.shape[0]))):
        if which == "westervelt-fused":
            s = nls.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=1500.0, source_frequency=0.5e6, fused=True, sponge=layer)
        else:
            s = ls.LinearSpectral3D(mesh, np.float64, fused=which == "linear-fused", sponge=layer)
        if layer is not None:
            assert s._sponge[0].numel() == 0 and layer.sigma_max == 0.0
        s.init()
        s.rk4(0.0, tf, dt, max_steps=6)
        res.append((s.u_sol(), s.v_sol()))
    assert np.max(np.abs(res[0][0])) > 0
    for u, v in res[1:]:
        assert np.array_equal(u.view(np.int64), res[0][0].view(np.int64)) and np.array_equal(v.view(np.int64), res[0][1].view(np.int64))


# ---- hipGraph replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["linear", "westervelt"])
def test_graph_replay_with_layer_matches_rk4(which):
    """rk4_graph with a layer: its launch takes fixed pointers only and is captured with the facet launch it follows -- the replayed
    steps (and the shorter last one through rk4) equal rk4's at the existing replay bar; and the layer was in the captured step."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, nls, sp = pkg("boxmesh"), pkg("linear_solver"), pkg("nonlinear_solver"), pkg("sponge")
    P, N, L = 3, 5, 0.012
    mesh = boxmesh.BoxMesh(P, N, length=L, perturb=0.12, seed=4)
    h = ls.time_step_parameters(mesh, P, 1500.0, 0.5e6, L)
    dt, _, _ = ls.snap_time_step(h, P, 1500.0, 0.5e6, L)
    tf = 14.5 * dt  # 14 full steps and a shorter last one
    sigma = _lateral(mesh, 1500.0)

    def make(layer):
        if which == "linear":
            return ls.LinearSpectral3D(mesh, np.float64, sponge=layer)
        return nls.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=1500.0, source_frequency=0.5e6, fused=True, sponge=layer)

    a, b, free = make(sp.SpongeLayer(sigma)), make(sp.SpongeLayer(sigma)), make(None)
    for s in (a, b, free):
        s.init()
    ta, sa = a.rk4(0.0, tf, dt)
    t1, s1 = b.rk4_graph(0.0, tf, dt, max_steps=6)  # captures
    t2, s2 = b.rk4_graph(t1, tf, dt)  # replays the same graph, then the short last step
    free.rk4_graph(0.0, tf, dt)
    assert sa == 15 and s1 == 6 and s1 + s2 == sa and abs(t2 - ta) < 1e-18 and len(b._graphs) == 1
    assert np.max(np.abs(a.u_sol())) > 0
    assert rel_l2(b.u_sol(), a.u_sol()) < 1e-13 and rel_l2(b.v_sol(), a.v_sol()) < 1e-13
    assert rel_l2(b.u_sol(), free.u_sol()) > 1e-3


# ---- two in-process ranks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 2, 1)], ids=["split-x", "split-y"])
def test_partitioned_linear_solver_with_layer(grid, fused):
    """Two ranks sharing cuda:0 in this process, the set-up exchange deferred to the driver (the layer is bound at its end, when each
    rank's lumped mass is complete): the lists hold owned dofs only and the term needs no exchange.  Split across x both ranks hold
    a part of every lateral layer; split across y each rank holds one y layer whole and the z layers in part, and the layer's launch
    runs next to the interior cells.  Against the single-rank run by lexicographic id."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, scat, utils, sp = pkg("boxmesh"), pkg("linear_solver"), pkg("scatterer"), pkg("utils"), pkg("sponge")
    P, cells, L, R, nsteps = 3, (4, 4, 4), 0.012, 2, 8
    meshes = [boxmesh.BoxMesh(P, cells, grid=grid, rank=r, length=L) for r in range(R)]
    serial = boxmesh.BoxMesh(P, cells, length=L)
    h = ls.time_step_parameters(serial, P, 1500.0, 0.5e6, L)
    dt, tf, _ = ls.snap_time_step(h, P, 1500.0, 0.5e6, L)
    layer = sp.SpongeLayer(_lateral(serial, 1500.0))  # one object for both ranks
    one = ls.LinearSpectral3D(serial, np.float64, fused=fused, sponge=layer)
    one.init()
    one.rk4(0.0, tf, dt, max_steps=nsteps)
    u_one, v_one = one.u_sol(), one.v_sol()
    od, gd = utils.compute_scatterer_data_all([m.index_map for m in meshes])
    wid = 8100 + 10 * grid[1] + int(fused)
    solvers = [ls.LinearSpectral3D(meshes[r], np.float64, comm=scat.NativeComm(local=(wid, R, r)), fused=fused, halo_plan=(od[r], gd[r]),
                                   defer_setup_exchange=True, sponge=layer) for r in range(R)]
    assert all(s._sponge is None for s in solvers)  # nothing is bound before the exchange has completed the mass
    _lockstep([s._setup for s in solvers])
    assert all(s._sponge[0].numel() > 0 for s in solvers)
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
        assert s.halo.health() == 0
    assert np.all(seen == 1)


def test_unbound_layer_is_an_error():
    """A solver whose deferred set-up exchange was never run has no coefficients: stepping it raises instead of skipping the layer."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, sp, lib_mod = pkg("boxmesh"), pkg("linear_solver"), pkg("sponge"), pkg("_lib")
    mesh = boxmesh.BoxMesh(2, (3, 3, 3), length=0.006)
    s = ls.LinearSpectral3D(mesh, np.float64, defer_setup_exchange=True, sponge=sp.SpongeLayer(_lateral(mesh, 1500.0)))
    s.init()
    with pytest.raises(lib_mod.FusGpuError, match="set-up exchange"):
        s.rk4(0.0, 1e-6, 1e-7, max_steps=1)


# ---- fp32 --------------------------------------------------------------------------------------------------------------------------
def test_fp32_linear_solver_with_layer():
    """The fused fp32 solver with a layer against the fp64 one.  The bar is the solver's own fp32 error: twice the fp32-to-fp64 distance
    of the LAYER-FREE solver on the same mesh and steps, measured here.  Measured on one MI355X, rel l2 (u, v): layer-free 7.90e-08,
    1.88e-07; with the layer 1.09e-07, 1.90e-07 (bars 1.58e-07, 3.76e-07)."""
    import torch

    torch.cuda.set_device(0)
    boxmesh, ls, sp = pkg("boxmesh"), pkg("linear_solver"), pkg("sponge")
    k = _LINEAR["box"]
    meshes = {np.dtype(ft).name: boxmesh.BoxMesh(k["P"], k["cells"], length=k["length"], dtype=ft) for ft in (np.float64, np.float32)}
    mesh = meshes["float64"]
    h = ls.time_step_parameters(mesh, k["P"], 1500.0, 0.5e6, mesh.length[0])
    dt, tf, _ = ls.snap_time_step(h, k["P"], 1500.0, 0.5e6, mesh.length[0])
    sigma = _lateral(mesh, 1500.0)
    out = {}
    for layered in (False, True):
        for ft in (np.float64, np.float32):
            s = ls.LinearSpectral3D(meshes[np.dtype(ft).name], ft, sponge=sp.SpongeLayer(sigma) if layered else None)
            s.init()
            s.rk4(0.0, tf, dt, max_steps=k["steps"])
            out[layered, np.dtype(ft).name] = (s.u_sol().astype(np.float64), s.v_sol().astype(np.float64))
    free = [rel_l2(out[False, "float32"][i], out[False, "float64"][i]) for i in (0, 1)]
    layer = [rel_l2(out[True, "float32"][i], out[True, "float64"][i]) for i in (0, 1)]
    print(f"fp32 to fp64, rel l2 (u, v): layer-free {free[0]:.3e} {free[1]:.3e}, with the layer {layer[0]:.3e} {layer[1]:.3e}")
    assert np.max(np.abs(out[True, "float64"][0])) > 0 and min(free) > 0
    assert layer[0] < 2 * free[0] and layer[1] < 2 * free[1]
