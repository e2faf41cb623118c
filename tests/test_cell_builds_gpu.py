"""Every shipped build of the constant-coefficient cell kernels against an fp64 model (tests/cell_model64.py):

    plan             stiffness_plan_kernel         y += K(cc) x                        csrc/stiffness_plan.hpp   builds 0 / 1 / 2 / 30
    rows             stiffness_plan_rows_kernel    the same, one slot per local row    csrc/stiffness_plan.hpp   fp64, P = 2..8, run tables
    affine           stiffness_plan_affine_kernel  G[c, q] = G[c, 0] w_q / w_0         csrc/stiffness_affine.hpp
    geom             stiffness_plan_geom_kernel    G from the cell vertices            csrc/stiffness_geom.hpp
    westervelt       westervelt_cell_kernel        b += K(c3) u + K(c4) v (+ M(c5) v^2,  m += M(c2) u  with MASS)      csrc/westervelt.hpp
    westervelt_geom  westervelt_cell_geom_kernel   the same, G and detJ from the cell vertices                        csrc/westervelt_geom.hpp

``MATRIX`` holds one case per instantiation the library compiles of these kernels (726: tests/test_cell_model64.py compares the list
with the kernel names of a device-only compile, without a GPU); ``template_key`` states which instantiation a case runs.  A case
steers the dispatch and asserts what can be observed of it: the plan cache's ``last_order`` (ORDERED), ``TUNE_PLAN_RUNS`` and
``fus_plan_encoding`` (RUNS), ``TUNE_PLAN_VARIANT`` (the build of stiffness_plan_kernel; a forced build bypasses the rows kernel),
``TUNE_PLAN_ROWS`` and the plan header's ``rows_consecutive`` (the rows kernel), the full call against ``stiffness_only`` (MASS).
The edge cases follow: one cell, no cell, an exactly full last batch, a dofmap with heavy collisions.

Every launch writes into views of buffers 16 elements longer, pre-filled with a sentinel: nothing may be written behind a vector.

The bars.  fp64: the project's ``TOL`` (rel l2 < 1e-12, rel max < 1e-11) against the fp64 model.  fp32: ``TOL`` as it stands AND the rule
of tests/test_nodal_builds_gpu.py,

    err_gpu <= 8 x max(e_cpu, 2^-23),    for rel l2 and for rel max separately, and with MASS for b and m separately,

``e_cpu`` being the fp32 CPU oracle's distance from the same model on the same once-rounded inputs.  Every case prints err_gpu, e_cpu
and their ratio (profiles/cell_builds_errors.log is one run's output: fp64 4e-17 .. 1.1e-15; fp32 ratios 0.16 .. 1.47 in rel l2 and
0.11 .. 3.29 in rel max, the in-kernel-geometry kernels highest, the general-G and affine kernels below 1.2 / 2.7).  Nothing here is
timed."""

import collections
import ctypes

import numpy as np
import pytest

import cell_model64 as model
from conftest import TOL, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 16, -7.25
FP32_MARGIN, FP32_FLOOR = 8.0, 2.0**-23

# per degree the smallest box with more than 2 x cells-per-batch cells (where the plan cache tries a cell order of its own) and a ragged
# last batch; no more than 4 x cells-per-batch, so the strip order is never tried (tests/test_nodal_builds_gpu.py)
SHAPES = {1: (5, 4, 7), 2: (4, 4, 4), 3: (4, 3, 3), 4: (3, 3, 3), 5: (5, 3, 1), 6: (11, 1, 1), 7: (9, 1, 1), 8: (7, 1, 1), 9: (7, 1, 1),
          10: (7, 1, 1)}
DTYPES = {"f64": np.float64, "f32": np.float32}
KERNEL = {"plan": "stiffness_plan_kernel", "rows": "stiffness_plan_rows_kernel", "affine": "stiffness_plan_affine_kernel",
          "geom": "stiffness_plan_geom_kernel", "westervelt": "westervelt_cell_kernel", "westervelt_geom": "westervelt_cell_geom_kernel"}
MODEL = {"plan": "general", "rows": "general", "affine": "affine", "geom": "geom", "westervelt": "westervelt", "westervelt_geom": "westervelt_geom"}
OUTPUTS = {None: ("y",), False: ("bs",), True: ("b", "m")}  # by MASS (None: a stiffness kernel)

# ``variant``: TUNE_PLAN_VARIANT for the family "plan" (0, 1, 2, 30), -1 (auto) for the others; ``mass``: None where the kernel has no MASS
Build = collections.namedtuple("Build", "family dtype P variant mass ordered runs")

# slabs of G in the ring of build 2 and of the Westervelt kernel (csrc/stiffness_plan.hpp: plan_g_ring)
G_RING = {1: 2, 2: 3, 3: 4, 4: 3, 5: 3, 6: 4, 7: 3, 8: 2, 9: 1, 10: 6}
ROWS_DEGREES = range(2, 9)  # csrc/dispatch_stiffness_plan.hip: plan_rows_ships


def _plan_build_args(dtype, P, variant):
    """(ALIAS, PADLDS, MINW, GPRE) of build ``variant`` of stiffness_plan_kernel (csrc/dispatch_stiffness_plan.hip)."""
    if variant == 1:
        return (True, True, 1, P + 1)
    if variant == 2:
        return (True, P != 8, 1, G_RING[P])
    if variant == 30 and dtype == "f32" and P <= 4:
        return (False, True, 5, P + 1)
    return (False, True, 1, P + 1)


def _plan_auto_variant(dtype, P):
    return (30 if P <= 4 else 1) if dtype == "f32" else (0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2)[P]


def _geom_flux_form(dtype, P):  # csrc/stiffness_geom.hpp: geom_flux_operator_form
    return P in ((2, 3, 6, 8, 9) if dtype == "f64" else (2, 3, 4))


def template_key(b):
    """(kernel, type, P, the template arguments between CPB and (ORDERED, RUNS), ORDERED, RUNS) of the instantiation that case ``b``
    launches: the dispatch tables of csrc/dispatch_*.hip, restated."""
    P = b.P
    if b.family == "plan":
        args = _plan_build_args(b.dtype, P, b.variant)
    elif b.family == "rows":
        args = _plan_build_args(b.dtype, P, _plan_auto_variant(b.dtype, P))
    elif b.family == "affine":
        args = (True, P > 4, 5 if P <= 4 else 1)
    elif b.family == "geom":
        args = (P >= 4, True, 1, P <= 5 and not (P >= 2 and _geom_flux_form(b.dtype, P)))
    elif b.family == "westervelt":
        ring = (P + 1 if P <= 3 else G_RING[P]) if b.mass else (G_RING[P] if P >= 6 else P + 1)
        args = (1, ring, b.mass)
    else:
        args = (1, b.mass)
    return (KERNEL[b.family], "double" if b.dtype == "f64" else "float", P, args, b.ordered, b.runs)


def plan_variants(dtype, P):
    """The forced builds of stiffness_plan_kernel whose template arguments differ: build 2 is build 1 where the ring is the whole slab
    (P <= 3), build 30 is build 0 in fp64 and in fp32 above P = 4."""
    return [v for v in (0, 1, 2, 30) if not (v == 2 and P <= 3) and not (v == 30 and (dtype == "f64" or P > 4))]


def _matrix():
    out = []
    for dtype in DTYPES:
        for P in sorted(SHAPES):
            axes = [(o, r) for o in (False, True) for r in (False, True)]
            out += [Build("plan", dtype, P, v, None, o, r) for v in plan_variants(dtype, P) for o, r in axes]
            if dtype == "f64" and P in ROWS_DEGREES:
                out += [Build("rows", dtype, P, -1, None, o, True) for o in (False, True)]
            out += [Build(f, dtype, P, -1, None, o, r) for f in ("affine", "geom") for o, r in axes]
            out += [Build(f, dtype, P, -1, m, o, r) for f in ("westervelt", "westervelt_geom") for m in (False, True) for o, r in axes]
    return out


MATRIX = _matrix()


def _id(b):
    mass = {None: "", False: "-stiff", True: "-mass"}[b.mass]
    return f"{b.family}-P{b.P}-{b.dtype}" + (f"-b{b.variant}" if b.family == "plan" else "") + mass + ("-ordered" if b.ordered else "-natural") + \
        ("-runs" if b.runs else "-lists")


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
    knobs = (lib.TUNE_PLAN_RUNS, lib.TUNE_PLAN_VARIANT, lib.TUNE_PLAN_ROWS)
    old, old_loc, old_plan = [lib.get_tuning(k) for k in knobs], ops._LOCALITY_ORDER, ops._USE_PLAN
    ops._PLANS.clear()
    ops.use_locality_order(True)
    ops.use_plan(True)
    yield
    for k, v in zip(knobs, old):
        lib.set_tuning(k, v)
    ops.use_locality_order(old_loc)
    ops.use_plan(old_plan)
    ops._PLANS.clear()


_cases = {}


def _case(kind, key, geometry):
    """One model per (kind, degree, type, shape): computed once, read-only (cell_model64 freezes its arrays)."""
    if (kind, key) not in _cases:
        _cases[kind, key] = model.model(kind, geometry())
    return _cases[kind, key]


def _box_case(family, P, shape, dtype):
    kind = MODEL[family]
    return _case(kind, (P, shape, np.dtype(dtype).name), lambda: (model.affine_box if kind == "affine" else model.box)(P, shape, dtype))


def _colliding_case(family, dtype):
    kind = MODEL[family]
    return _case(kind, ("colliding", np.dtype(dtype).name), lambda: model.colliding(dtype, affine=kind == "affine"))


def _td(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases are read-only)


class _Launch:
    """The operator of a case and its device arguments; ``rows``: a permutation of the cells applied to the rows of every per-cell
    array.  ``apply(mass)`` launches once into views of buffers GUARD elements longer, pre-filled with a sentinel, and returns
    {output: (the vector on the host, whether its guard is untouched)} for the outputs of ``OUTPUTS[mass]``."""

    def __init__(self, ops, c, family, rows=None, ncells=None):
        self.ops, self.c, self.family = ops, c, family
        P, D, dtype = c["P"], _td(c["D"]), c["dtype"]
        self.cell = lambda k: _td(c[k] if rows is None else c[k][rows])[:ncells]  # noqa: E731
        self.dofmap = self.cell("dofmap")
        if family in ("plan", "rows"):
            self.op, self.geometry = ops.stiffness_operator(P, D, dtype), (self.cell("G"),)
        elif family == "affine":
            self.op, self.geometry = ops.stiffness_operator(P, D, dtype, affine_weights=c["w3"]), (self.cell("G"),)
        elif family == "geom":  # (a cell range hands its rows of x_dofs in the G position)
            self.op = ops.stiffness_operator(P, D, dtype, geometry=(_td(c["x_dofs"]), _td(c["x_g"]), _td(c["pts"]), _td(c["wts"])))
            self.geometry = (self.cell("x_dofs"),)
        elif family == "westervelt":
            self.op, self.geometry = ops.westervelt_cell_operator(P, D, dtype), (self.cell("G"), self.cell("detJ"))
        else:
            self.op = ops.westervelt_cell_operator(P, D, dtype, geometry=(_td(c["x_g"]), _td(c["pts"]), _td(c["wts"])))
            self.geometry = (self.cell("x_dofs"),)

    def apply(self, mass=None):
        import torch

        c, n = self.c, self.c["ndofs"]
        tdt = torch.float64 if c["dtype"] == np.float64 else torch.float32
        bufs = {k: torch.full((n + GUARD,), SENTINEL, dtype=tdt, device="cuda") for k in OUTPUTS[mass]}
        out = {k: buf[:n] for k, buf in bufs.items()}
        for k, v in out.items():
            v.copy_(_td(c["out"][k]["y0"]))
        if mass is None:
            self.op(_td(c["x"]), self.cell("cc"), out["y"], *self.geometry, self.dofmap)
        elif mass:
            self.op(_td(c["u"]), _td(c["v"]), self.cell("c2"), self.cell("c3"), self.cell("c4"), self.cell("c5"), out["b"], out["m"],
                    *self.geometry, self.dofmap)
        else:
            self.op.stiffness_only(_td(c["u"]), _td(c["v"]), self.cell("c3"), self.cell("c4"), out["bs"], self.geometry[0], self.dofmap)
        torch.cuda.synchronize()
        return {k: (out[k].cpu().numpy(), bool((bufs[k][n:] == SENTINEL).all().item())) for k in out}

    def plan(self):
        """The one cached plan: its workspace."""
        (ws, *_), = self.ops._PLANS._plans.values()
        return ws

    def encoding(self, lib):
        """(batches, batches with a run table, whether a launch of this type reads the tables) of the one cached plan."""
        nb, nr, r64, r32 = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
        assert lib.load().fus_plan_encoding(self.plan().data_ptr(), ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(r64), ctypes.byref(r32)) == 0
        return nb.value, nr.value, bool((r64 if self.c["dtype"] == np.float64 else r32).value)

    def rows_consecutive(self):
        """``rows_consecutive`` of the plan's header (tests/test_plan_rows_gpu.py::_header)."""
        return int(self.plan()[:256].cpu().numpy().view(np.int64)[8])


def _check(got, rec, what):
    """``got`` against the model of one output vector at the bars of its type, the figures printed first."""
    tol = TOL[np.dtype(rec["dtype"])]
    e2, em = rel_l2(got, rec["ref"]), rel_max(got, rec["ref"])
    line = f"{what}: err_gpu l2 {e2:.3e} max {em:.3e}"
    if rec["e_cpu"] is not None:
        f2, fm = (max(e, FP32_FLOOR) for e in rec["e_cpu"])
        line += f"; e_cpu l2 {rec['e_cpu'][0]:.3e} max {rec['e_cpu'][1]:.3e}; ratio l2 {e2 / f2:.2f} max {em / fm:.2f} (bar {FP32_MARGIN:g})"
    print(line)
    assert e2 < tol["l2"] and em < tol["mx"], f"{line}; TOL l2 {tol['l2']} max {tol['mx']}"
    if rec["dtype"] == np.float32:
        b2, bm = (FP32_MARGIN * max(e, FP32_FLOOR) for e in rec["e_cpu"])
        assert e2 <= b2 and em <= bm, f"{line}; bars l2 {b2:.3e} max {bm:.3e}"


def _check_apply(c, results, what):
    """Every output of a launch: the guard, that something of the size of ``add`` was ADDED on a non-zero y0, the bars."""
    for k, (got, guard) in results.items():
        rec = c["out"][k]
        assert guard, f"{what}: the launch wrote behind {k}"
        assert np.max(np.abs(rec["y0"])) > 0 and np.max(np.abs(got - rec["y0"])) > 0.5 * np.max(np.abs(rec["add"])), f"{what}: nothing was ADDED to {k}"
    for k, (got, _) in results.items():
        _check(got, c["out"][k], f"{what} {k}")


def _steer(lib, family, variant=-1, runs=None):
    lib.set_tuning(lib.TUNE_PLAN_VARIANT, variant)
    lib.set_tuning(lib.TUNE_PLAN_ROWS, 1 if family == "rows" else 0)
    if runs is not None:
        lib.set_tuning(lib.TUNE_PLAN_RUNS, 2 if runs else 0)


# ---- (a) the build matrix --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", MATRIX, ids=[_id(b) for b in MATRIX])
def test_every_build_matches_the_fp64_model(gpu, b):
    """One case per compiled instantiation.  ORDERED: the cells are handed over as "the even ones, then the odd ones", an order the plan
    cache replaces by one of its own at every degree (tests/test_nodal_builds_gpu.py).  RUNS: ``TUNE_PLAN_RUNS`` 2 makes every launch
    read the run tables, 0 builds the plan without them.  The build of stiffness_plan_kernel: ``TUNE_PLAN_VARIANT``, which also keeps the
    launch off the rows kernel; the rows kernel: variant -1, ``TUNE_PLAN_ROWS`` 1, run tables, a plan whose header says that every row
    is consecutive.  MASS: the full call; without, ``stiffness_only``."""
    ops, lib = gpu
    c = _box_case(b.family, b.P, SHAPES[b.P], DTYPES[b.dtype])
    nc, cpb = c["ncells"], lib.load().fus_plan_entities_per_batch((b.P + 1) ** 3)
    assert 2 * cpb < nc <= 4 * cpb and nc % cpb != 0
    rows = np.concatenate((np.arange(0, nc, 2), np.arange(1, nc, 2))) if b.ordered else None
    _steer(lib, b.family, b.variant, b.runs)
    launch = _Launch(ops, c, b.family, rows)
    results = launch.apply(b.mass)
    # which build ran
    assert (ops._PLANS.last_order is not None) == b.ordered, "the plan cache did not keep the intended cell order"
    nbatch, with_runs, reads = launch.encoding(lib)
    assert lib.get_tuning(lib.TUNE_PLAN_RUNS) == (2 if b.runs else 0) and nbatch == -(-nc // cpb)
    assert (with_runs, reads) == ((nbatch, True) if b.runs else (0, False)), f"{with_runs} of {nbatch} batches carry a run table, read: {reads}"
    assert lib.get_tuning(lib.TUNE_PLAN_VARIANT) == b.variant and lib.get_tuning(lib.TUNE_PLAN_ROWS) == (b.family == "rows")
    if b.family == "rows":
        assert b.dtype == "f64" and b.runs and b.P in ROWS_DEGREES and launch.rows_consecutive() == 1
    _check_apply(c, results, _id(b))


# ---- (b) edge cases --------------------------------------------------------------------------------------------------------------------
def _edge_builds(degrees, rows=True):
    """(family, type, P, MASS) of the edge cases: every kernel in both types, with and without MASS where it exists.  "plan" is the
    auto build of stiffness_plan_kernel (``TUNE_PLAN_ROWS`` 0), "rows" the rows kernel where it ships."""
    out = []
    for P in degrees:
        for dtype in DTYPES:
            out += [(f, dtype, P, None) for f in ("plan", "affine", "geom")]
            if rows and dtype == "f64" and P in ROWS_DEGREES:
                out.append(("rows", dtype, P, None))
            out += [(f, dtype, P, m) for f in ("westervelt", "westervelt_geom") for m in (False, True)]
    return out


def _edge_id(e):
    return f"{e[0]}-P{e[2]}-{e[1]}" + {None: "", False: "-stiff", True: "-mass"}[e[3]]


def _edge(gpu, e, c, what):
    ops, lib = gpu
    family, dtype, P, mass = e
    _steer(lib, family)
    launch = _Launch(ops, c, family)
    results = launch.apply(mass)
    if family == "rows":
        assert lib.get_tuning(lib.TUNE_PLAN_RUNS) != 0 and launch.encoding(lib)[2] and launch.rows_consecutive() == 1
    _check_apply(c, results, f"{_edge_id(e)} {what}")


ONE_CELL = _edge_builds((1, 4, 10))


@pytest.mark.parametrize("e", ONE_CELL, ids=[_edge_id(e) for e in ONE_CELL])
def test_one_cell(gpu, e):
    """One cell: one batch with 63 of 64 (P = 1), 9 of 10 (P = 4), 1 of 2 (P = 10) cell slots idle."""
    ops, lib = gpu
    c = _box_case(e[0], e[2], (1, 1, 1), DTYPES[e[1]])
    assert c["ncells"] == 1 < lib.load().fus_plan_entities_per_batch((e[2] + 1) ** 3)
    _edge(gpu, e, c, "one cell")
    assert ops._PLANS.last_order is None


ZERO_CELLS = _edge_builds((4,), rows=False)


@pytest.mark.parametrize("e", ZERO_CELLS, ids=[_edge_id(e) for e in ZERO_CELLS])
def test_zero_cells(gpu, e):
    """An empty cell range: nothing is raised, nothing is launched, every output is unchanged to the bit, no plan is cached."""
    ops, lib = gpu
    family, dtype, P, mass = e
    c = _box_case(family, P, (1, 1, 1), DTYPES[dtype])
    _steer(lib, family)
    launch = _Launch(ops, c, family, ncells=0)
    assert launch.dofmap.shape[0] == 0 and all(g.shape[0] == 0 for g in launch.geometry) and launch.cell("c3" if mass is not None else "cc").numel() == 0
    for k, (got, guard) in launch.apply(mass).items():
        assert guard and np.array_equal(got, c["out"][k]["y0"]), k
    assert len(ops._PLANS._plans) == 0


FULL_BATCH = [(e, shape) for P, shape in ((4, (5, 2, 2)), (7, (3, 2, 2))) for e in _edge_builds((P,))]


@pytest.mark.parametrize("e,shape", FULL_BATCH, ids=[_edge_id(e) for e, _ in FULL_BATCH])
def test_exactly_full_last_batch(gpu, e, shape):
    """P = 4: 20 cells in two batches of 10; P = 7: 12 cells in three batches of 4."""
    ops, lib = gpu
    c = _box_case(e[0], e[2], shape, DTYPES[e[1]])
    cpb = lib.load().fus_plan_entities_per_batch((e[2] + 1) ** 3)
    assert c["ncells"] % cpb == 0 and c["ncells"] > cpb
    _edge(gpu, e, c, f"{c['ncells']} cells in full batches of {cpb}")


COLLIDING = _edge_builds((3,), rows=False)


@pytest.mark.parametrize("e", COLLIDING, ids=[_edge_id(e) for e in COLLIDING])
def test_colliding_dofmap(gpu, e):
    """Scatter-add under heavy collisions (as tests/test_operators_gpu.py::test_colliding_dofmap): P = 3, 37 cells whose dofmap rows
    are random integers in [0, 50) -- dofs repeat inside a cell and every batch touches every dof; the geometry is a tiled 2 x 2 x 2
    mesh (the affine kernel: the tiled affine box).  No row of such a dofmap is consecutive: the rows kernel is never chosen for it."""
    c = _colliding_case(e[0], DTYPES[e[1]])
    assert c["ncells"] == 37 and c["ndofs"] == 50 and c["dofmap"].max() < 50
    _edge(gpu, e, c, "colliding dofmap")
