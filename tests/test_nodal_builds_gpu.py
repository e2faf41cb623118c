"""Every shipped build of the two nodal cell kernels against an fp64 model (tests/nodal_model64.py):

    stiffness_plan_geom_nodal_kernel    y += K(cc kappa) x                      csrc/stiffness_geom_nodal.hpp
    westervelt_cell_geom_nodal_kernel   b += K(c3 kappa3) u + K(c4 kappa4) v    csrc/westervelt_geom_nodal.hpp

Each ships as 80 instantiations: P = 1..10 x {fp64, fp32} x (ORDERED, RUNS).  The build matrix launches all of them and asserts which
one ran: the plan cache's ``last_order`` (ORDERED), ``fus_plan_encoding`` and the knob ``TUNE_PLAN_RUNS`` (RUNS).  The edge cases (one
cell, no cell, an exactly full last batch, a dofmap with heavy collisions) and an in-place update of the coefficients follow.

The bars.  fp64: the project's ``TOL`` (rel l2 < 1e-12, rel max < 1e-11) against the fp64 model.  fp32: ``TOL`` as it stands AND

    err_gpu <= 8 x max(e_cpu, 2^-23),    for rel l2 and for rel max separately,

where ``err_gpu`` and ``e_cpu`` are the distances of the kernel's result and of the fp32 CPU oracle's result from the same fp64 model on
the same once-rounded inputs.  2^-23 is the unit spacing of the type: the inputs are rounded once, no fp32 result can be expected
below it.  8: the kernel forms the Jacobian, its inverse and the factors in fp32 inside the launch and sums in another order, the
oracle reads a G rounded once; both are O(eps) with modest constants, and 8 is under one decimal digit.  e_cpu is 4e-8 .. 1.3e-7
(l2) and up to 2.7e-7 (max) on these inputs, so the bar sits near 1e-6 / 2e-6: 10 x and 50 x below ``TOL``.  Every case prints err_gpu,
e_cpu and their ratio (profiles/nodal_builds_errors.log is one run's output).  Nothing here is timed."""

import ctypes

import numpy as np
import pytest

import nodal_model64 as model
from conftest import TOL, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 16, -7.25
FP32_MARGIN, FP32_FLOOR = 8.0, 2.0**-23

# per degree the smallest box with more than 2 x cells-per-batch cells (where the plan cache tries a cell order of its own) and a ragged
# last batch; no more than 4 x cells-per-batch, so the strip order is never tried.  (cells, cells per batch) = (140, 64), (64, 28),
# (36, 16), (27, 10), (15, 7), (11, 5), (9, 4), (7, 3), (7, 2), (7, 2)
SHAPES = {1: (5, 4, 7), 2: (4, 4, 4), 3: (4, 3, 3), 4: (3, 3, 3), 5: (5, 3, 1), 6: (11, 1, 1), 7: (9, 1, 1), 8: (7, 1, 1), 9: (7, 1, 1),
          10: (7, 1, 1)}
KERNELS = ("stiffness", "pair")
DTYPES = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    torch.cuda.set_device(0)
    return pkg("operators"), pkg("_lib")


@pytest.fixture(autouse=True)
def _restore(gpu):
    ops, lib = gpu
    old_runs, old_loc = lib.get_tuning(lib.TUNE_PLAN_RUNS), ops._LOCALITY_ORDER
    ops._PLANS.clear()
    ops.use_locality_order(True)
    yield
    lib.set_tuning(lib.TUNE_PLAN_RUNS, old_runs)
    ops.use_locality_order(old_loc)
    ops._PLANS.clear()


_cases = {}


def _case(kernel, key, geometry):
    """One model per (kernel, geometry, type): computed once, read-only (nodal_model64 freezes its arrays)."""
    if (kernel, key) not in _cases:
        _cases[kernel, key] = model.MODELS[kernel](geometry())
    return _cases[kernel, key]


def _box_case(kernel, P, shape, dtype):
    return _case(kernel, (P, shape, np.dtype(dtype).name), lambda: model.box(P, shape, dtype))


def _td(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases are read-only)


def _operator(ops, c):
    geometry = (_td(c["x_g"]), _td(c["pts"]), _td(c["wts"]))
    if c["kind"] == "stiffness":
        return ops.stiffness_operator(c["P"], _td(c["D"]), c["dtype"], geometry=(_td(c["x_dofs"]),) + geometry, nodal=_td(c["kappa"]))
    return ops.westervelt_cell_operator(c["P"], _td(c["D"]), c["dtype"], geometry=geometry, nodal=(_td(c["k3"]), _td(c["k4"])))


def _constants(c):
    return (c["cc"],) if c["kind"] == "stiffness" else (c["c3"], c["c4"])


class _Launch:
    """The operator of a case and its device arguments; ``rows``: a permutation of the cells applied to the rows of the dofmap, of
    x_dofs and of the cell constants.  ``apply()`` launches once into a view of a buffer GUARD elements longer, pre-filled with a
    sentinel, and returns y on the host and whether the guard is untouched."""

    def __init__(self, ops, c, rows=None, ncells=None):
        pick = lambda a: a if rows is None else a[rows]  # noqa: E731
        self.ops, self.c = ops, c
        self.op = _operator(ops, c)
        self.vectors = [_td(c[k]) for k in (("x",) if c["kind"] == "stiffness" else ("u", "v"))]
        self.constants = [_td(pick(a))[:ncells] for a in _constants(c)]
        self.x_dofs, self.dofmap = _td(pick(c["x_dofs"]))[:ncells], _td(pick(c["dofmap"]))[:ncells]

    def apply(self, y0=None):
        import torch

        n = self.c["ndofs"]
        buf = torch.full((n + GUARD,), SENTINEL, dtype=self.vectors[0].dtype, device="cuda")
        y = buf[:n]
        y.copy_(_td(self.c["y0"] if y0 is None else y0))
        if self.c["kind"] == "stiffness":  # (a cell range hands its rows of x_dofs in the G position)
            self.op(*self.vectors, *self.constants, y, self.x_dofs, self.dofmap)
        else:
            self.op.stiffness_only(*self.vectors, *self.constants, y, self.x_dofs, self.dofmap)
        torch.cuda.synchronize()
        return y.cpu().numpy(), bool((buf[n:] == SENTINEL).all().item())

    def encoding(self, lib):
        """(batches, batches with a run table, whether a launch of this type reads the tables) of the one cached plan."""
        (ws, *_), = self.ops._PLANS._plans.values()
        nb, nr, r64, r32 = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
        assert lib.load().fus_plan_encoding(ws.data_ptr(), ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(r64), ctypes.byref(r32)) == 0
        return nb.value, nr.value, bool((r64 if self.c["dtype"] == np.float64 else r32).value)


def _fp32_bars(c):
    """(l2, max) bars of an fp32 case next to TOL: FP32_MARGIN x max(e_cpu, FP32_FLOOR)."""
    return tuple(FP32_MARGIN * max(e, FP32_FLOOR) for e in c["e_cpu"])


def _check(got, ref, c, what):
    """``got`` against ``ref`` at the bars of the case, the figures printed first."""
    tol = TOL[np.dtype(c["dtype"])]
    e2, em = rel_l2(got, ref), rel_max(got, ref)
    line = f"{what}: err_gpu l2 {e2:.3e} max {em:.3e}"
    if c["e_cpu"] is not None:
        f2, fm = (max(e, FP32_FLOOR) for e in c["e_cpu"])
        line += f"; e_cpu l2 {c['e_cpu'][0]:.3e} max {c['e_cpu'][1]:.3e}; ratio l2 {e2 / f2:.2f} max {em / fm:.2f} (bar {FP32_MARGIN:g})"
    print(line)
    assert e2 < tol["l2"] and em < tol["mx"], f"{line}; TOL l2 {tol['l2']} max {tol['mx']}"
    if c["dtype"] == np.float32:
        b2, bm = _fp32_bars(c)
        assert e2 <= b2 and em <= bm, f"{line}; bars l2 {b2:.3e} max {bm:.3e}"


def _check_apply(c, got, guards, what):
    assert guards, f"{what}: the launch wrote behind y"
    assert np.max(np.abs(c["y0"])) > 0 and np.max(np.abs(got - c["y0"])) > 0.5 * np.max(np.abs(c["add"])), f"{what}: nothing was ADDED to y"
    _check(got, c["ref"], c, what)


# ---- (a) the build matrix --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("runs", [0, 2], ids=["lists", "run-tables"])
@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "ordered"])
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("P", sorted(SHAPES))
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_build_matches_the_fp64_model(gpu, kernel, P, dtype, ordered, runs):
    """Both kernels x P = 1..10 x {fp64, fp32} x (ORDERED, RUNS).  ORDERED: the cells are handed over as "the even ones, then the odd
    ones" -- an order the plan cache replaces by one of its own at every degree (its rule: the distinct dofs of the min-dof-sorted plan
    are below 0.97 x the unsorted one's; here 0.64 .. 0.961 for P = 1 .. 10; a random order is not replaced at P >= 7 on meshes this
    small).  RUNS: ``TUNE_PLAN_RUNS`` 2 makes every launch read the run tables, 0 builds the plan without them."""
    ops, lib = gpu
    c = _box_case(kernel, P, SHAPES[P], DTYPES[dtype])
    nc, cpb = c["ncells"], lib.load().fus_plan_entities_per_batch((P + 1) ** 3)
    assert 2 * cpb < nc <= 4 * cpb and nc % cpb != 0
    rows = np.concatenate((np.arange(0, nc, 2), np.arange(1, nc, 2))) if ordered else None
    lib.set_tuning(lib.TUNE_PLAN_RUNS, runs)
    launch = _Launch(ops, c, rows)
    got, guards = launch.apply()
    # which build ran
    assert (ops._PLANS.last_order is not None) == ordered, "the plan cache did not keep the intended cell order"
    nbatch, with_runs, reads = launch.encoding(lib)
    assert lib.get_tuning(lib.TUNE_PLAN_RUNS) == runs and nbatch == -(-nc // cpb)
    assert (with_runs, reads) == ((nbatch, True) if runs else (0, False)), f"{with_runs} of {nbatch} batches carry a run table, read: {reads}"
    _check_apply(c, got, guards, f"{kernel} P={P} {dtype} ordered={int(ordered)} runs={runs}")


# ---- (b) edge cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("P", [1, 4, 10])
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_cell(gpu, kernel, P, dtype):
    """One cell: one batch with 63 of 64 (P = 1), 9 of 10 (P = 4), 1 of 2 (P = 10) cell slots idle."""
    ops, lib = gpu
    c = _box_case(kernel, P, (1, 1, 1), DTYPES[dtype])
    assert c["ncells"] == 1 < lib.load().fus_plan_entities_per_batch((P + 1) ** 3)
    got, guards = _Launch(ops, c).apply()
    assert ops._PLANS.last_order is None
    _check_apply(c, got, guards, f"{kernel} P={P} {dtype} one cell")


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("kernel", KERNELS)
def test_zero_cells(gpu, kernel, dtype):
    """An empty cell range: nothing is raised, nothing is launched, y is unchanged to the bit."""
    ops, _ = gpu
    c = _box_case(kernel, 4, (1, 1, 1), DTYPES[dtype])
    launch = _Launch(ops, c, ncells=0)
    assert launch.dofmap.shape[0] == 0 and all(k.numel() == 0 for k in launch.constants)
    got, guards = launch.apply()
    assert guards and np.array_equal(got, c["y0"]) and len(ops._PLANS._plans) == 0


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("P,shape", [(4, (5, 2, 2)), (7, (3, 2, 2))], ids=["P4-20-cells", "P7-12-cells"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_exactly_full_last_batch(gpu, kernel, P, shape, dtype):
    ops, lib = gpu
    c = _box_case(kernel, P, shape, DTYPES[dtype])
    cpb = lib.load().fus_plan_entities_per_batch((P + 1) ** 3)
    assert c["ncells"] % cpb == 0 and c["ncells"] > cpb
    got, guards = _Launch(ops, c).apply()
    _check_apply(c, got, guards, f"{kernel} P={P} {dtype} {c['ncells']} cells in full batches of {cpb}")


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("kernel", KERNELS)
def test_colliding_dofmap(gpu, kernel, dtype):
    """Scatter-add under heavy collisions (as tests/test_operators_gpu.py::test_colliding_dofmap): P = 3, 37 cells whose dofmap rows
    are random integers in [0, 50) -- dofs repeat inside a cell and every batch touches every dof; the geometry is a tiled 2 x 2 x 2 mesh."""
    ops, _ = gpu
    c = _case(kernel, ("colliding", np.dtype(DTYPES[dtype]).name), lambda: model.colliding(DTYPES[dtype]))
    assert c["ncells"] == 37 and c["ndofs"] == 50 and c["dofmap"].max() < 50
    got, guards = _Launch(ops, c).apply()
    _check_apply(c, got, guards, f"{kernel} P=3 {dtype} colliding dofmap")


# ---- (c) the coefficients are read on every launch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P,dtype", [(4, "f64"), (5, "f32")], ids=["P4-f64", "P5-f32"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_in_place_coefficient_update(gpu, kernel, P, dtype):
    """``op.nodal`` times 2 in place (exact in binary): the next apply of the same operator on the same plan adds twice what the
    previous one added.  Both applies start from y = 0, so what they return IS what they added, and the errors are measured at the
    bars of the case against twice the first result and against twice the model."""
    ops, _ = gpu
    c = _box_case(kernel, P, SHAPES[P], DTYPES[dtype])
    launch = _Launch(ops, c)
    zero = np.zeros_like(c["y0"])
    first, g1 = launch.apply(zero)
    for k in ((launch.op.nodal,) if kernel == "stiffness" else launch.op.nodal):
        k.mul_(2)
    second, g2 = launch.apply(zero)
    assert g1 and g2 and len(ops._PLANS._plans) == 1
    what = f"{kernel} P={P} {dtype} coefficients doubled in place"
    assert np.max(np.abs(first)) > 0.5 * np.max(np.abs(c["add"]))
    _check(first, c["add"], c, f"{what}: first apply against the model")
    _check(second, 2.0 * first.astype(np.float64), c, f"{what}: second apply against twice the first")
    _check(second, 2.0 * c["add"], c, f"{what}: second apply against twice the model")
