"""Every shipped build of the mass, column and gradient cell kernels against an fp64 model (tests/cell_model64.py):

    gradient   gradient_plan_geom_kernel   y3 += C(c) x, the geometry from the cell vertices   csrc/gradient_geom.hpp   80
    col        stiffness_col_kernel        y += K(cc) x without a plan                          csrc/stiffness.hpp       40, x TUNE_XCD_REMAP 0 / 1
    mass_plan  mass_plan_kernel            y += M(c) x with a batch plan                        csrc/mass.hpp            36
    mass       mass_kernel                 the same, one thread per entry                       csrc/mass.hpp             4

tests/cell_op_builds.py holds one case per compiled instantiation (160: tests/test_cell_model64.py compares the list with the kernel
names of a device-only compile, without a GPU) and the shapes.  A case steers the dispatch and asserts what can be observed of it:
``TUNE_STIFFNESS_VARIANT`` / ``TUNE_XCD_REMAP`` and that no plan was built (col); the plan cache's ``last_order``, ``TUNE_PLAN_RUNS``
and ``fus_plan_encoding`` (gradient, mass_plan); the explicit (N, epb) of the C ABI calls, whose bucket of the EPT ladder
tests/test_cell_model64.py pins, and ``ops.mass_kernel_name`` on the Python route (mass_plan); the entry count on either side of 2^31 - 1
(mass).  The edge cases follow: one cell, no cell, an exactly full last batch, a dofmap with heavy collisions.

Every launch writes into views of buffers 16 elements longer, pre-filled with a sentinel: nothing may be written behind a vector.

The bars are those of tests/test_cell_builds_gpu.py.  fp64: ``TOL`` against the fp64 model.  fp32: ``TOL`` AND

    err_gpu <= 8 x max(e_bar, 2^-23),    for rel l2 and for rel max separately, per output vector,

``e_bar`` being the fp32 CPU reference's distance from the same model on the same once-rounded inputs (for the gradient capped at two
units: tests/cell_model64.py).  Every case prints err_gpu, e_cpu and their ratio (profiles/cell_op_builds_errors.log is one run's
output: fp64 4.3e-17 .. 1.0e-15; fp32 ratios in rel l2 / rel max: column 0.45 .. 1.10 / 0.65 .. 2.05, planned mass 0.23 .. 0.47 /
0.12 .. 1.00, mass_kernel 0.26 .. 1.06 / 0.31 .. 1.13, gradient 0.25 .. 1.07 / 0.19 .. 1.27).  Nothing here is timed, but the 2^31-entry
case prints how long it took (0.4 s in fp64, 0.1 s in fp32)."""

import ctypes
import time

import numpy as np
import pytest

import cell_model64 as model
import cell_op_builds as ob
from conftest import TOL, pkg, rel_l2, rel_max
from test_cell_builds_gpu import FP32_FLOOR, FP32_MARGIN, GUARD, SENTINEL, SHAPES

pytestmark = pytest.mark.gpu

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
    knobs = (lib.TUNE_PLAN_RUNS, lib.TUNE_STIFFNESS_VARIANT, lib.TUNE_XCD_REMAP)
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
    """One model per (kind, geometry): computed once, read-only (cell_model64 freezes its arrays)."""
    if (kind, key) not in _cases:
        _cases[kind, key] = model.model(kind, geometry())
    return _cases[kind, key]


def _box_case(kind, P, shape, dtype):
    return _case(kind, (P, tuple(shape), np.dtype(dtype).name), lambda: model.box(P, shape, dtype))


def _facet_case(P, shape, dtype):
    return _case("facet_mass", (P, tuple(shape), np.dtype(dtype).name), lambda: model.facet_box(P, shape, dtype))


def _colliding_case(kind, dtype):
    return _case(kind, ("colliding", np.dtype(dtype).name), lambda: model.colliding(dtype))


def _td(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases are read-only)


def _tdt(c):
    import torch

    return torch.float64 if c["dtype"] == np.float64 else torch.float32


def _guarded(c, keys):
    """Per output a buffer GUARD elements longer, pre-filled with the sentinel, and its view holding y0."""
    import torch

    n = c["ndofs"]
    bufs = {k: torch.full((n + GUARD,), SENTINEL, dtype=_tdt(c), device="cuda") for k in keys}
    out = {k: buf[:n] for k, buf in bufs.items()}
    for k, v in out.items():
        v.copy_(_td(c["out"][k]["y0"]))
    return bufs, out


def _collect(c, bufs, out):
    import torch

    torch.cuda.synchronize()
    n = c["ndofs"]
    return {k: (out[k].cpu().numpy(), bool((bufs[k][n:] == SENTINEL).all().item())) for k in out}


def _check(got, rec, what, ref=None):
    """``got`` against the model of one output vector at the bars of its type, the figures printed first.  ``ref``: another reference
    than the record's (y0 + 2 add of a second launch): ``TOL`` alone."""
    tol = TOL[np.dtype(rec["dtype"])]
    target = rec["ref"] if ref is None else ref
    e2, em = rel_l2(got, target), rel_max(got, target)
    line = f"{what}: err_gpu l2 {e2:.3e} max {em:.3e}"
    fp32 = rec["dtype"] == np.float32 and ref is None
    if fp32:
        f2, fm = (max(e, FP32_FLOOR) for e in rec.get("e_bar", rec["e_cpu"]))  # (the general kind has no cap: e_cpu itself)
        line += (f"; e_cpu l2 {rec['e_cpu'][0]:.3e} max {rec['e_cpu'][1]:.3e}; ratio l2 {e2 / max(rec['e_cpu'][0], FP32_FLOOR):.2f} "
                 f"max {em / max(rec['e_cpu'][1], FP32_FLOOR):.2f}; against the bar's e l2 {e2 / f2:.2f} max {em / fm:.2f} (bar {FP32_MARGIN:g})")
    print(line)
    assert e2 < tol["l2"] and em < tol["mx"], f"{line}; TOL l2 {tol['l2']} max {tol['mx']}"
    if fp32:
        assert e2 <= FP32_MARGIN * f2 and em <= FP32_MARGIN * fm, f"{line}; bars l2 {FP32_MARGIN * f2:.3e} max {FP32_MARGIN * fm:.3e}"


def _check_apply(c, results, what):
    """Every output of a launch: the guard, that something of the size of ``add`` was ADDED on a non-zero y0, the bars."""
    for k, (got, guard) in results.items():
        rec = c["out"][k]
        assert guard, f"{what}: the launch wrote behind {k}"
        assert np.max(np.abs(rec["y0"])) > 0 and np.max(np.abs(got - rec["y0"])) > 0.5 * np.max(np.abs(rec["add"])), f"{what}: nothing was ADDED to {k}"
    for k, (got, _) in results.items():
        _check(got, c["out"][k], f"{what} {k}")


def _rows(c, rows, k, ncells=None):
    return _td(c[k] if rows is None else c[k][rows])[:ncells]


def _encoding(lib, ws, dtype):
    """(batches, batches with a run table, whether a launch of this type reads the tables) of the plan at ``ws``."""
    nb, nr, r64, r32 = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    assert lib.load().fus_plan_encoding(ws.data_ptr(), ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(r64), ctypes.byref(r32)) == 0
    return nb.value, nr.value, bool((r64 if np.dtype(dtype) == np.float64 else r32).value)


# ---- the launches ----------------------------------------------------------------------------------------------------------------------
def _gradient(ops, c, rows=None, ncells=None):
    """One launch of the gradient operator into the [3, ndofs] view of a [3, ndofs + GUARD] buffer (ystride > ndofs); the cells in the
    order ``rows`` (dofmap, x_dofs and constants alike)."""
    import torch

    n = c["ndofs"]
    x_dofs = np.array((c["x_dofs"] if rows is None else c["x_dofs"][rows])[:ncells], order="C")  # (a copy: the cases are read-only)
    op = ops.gradient_operator(c["P"], np.array(c["D"]).flatten(), c["dtype"], geometry=(x_dofs, np.array(c["x_g"]), np.array(c["pts"]), np.array(c["wts"])))
    buf = torch.full((3, n + GUARD), SENTINEL, dtype=_tdt(c), device="cuda")
    y3 = buf[:, :n]
    y3.copy_(_td(np.stack([c["out"][k]["y0"] for k in model.COMPONENTS])))
    assert y3.stride(0) == n + GUARD > n
    op(_td(c["x"]), _rows(c, rows, "cc", ncells), y3, _rows(c, rows, "dofmap", ncells))
    torch.cuda.synchronize()
    got = y3.cpu().numpy()
    return {k: (got[d], bool((buf[d, n:] == SENTINEL).all().item())) for d, k in enumerate(model.COMPONENTS)}


def _col(ops, lib, c, target, remap, ncells=None):
    """One launch of the plan-free stiffness apply with ~``target``-thread workgroups."""
    ops.use_plan(False)
    lib.set_tuning(lib.TUNE_STIFFNESS_VARIANT, 1 if target == 128 else 0)
    lib.set_tuning(lib.TUNE_XCD_REMAP, remap)
    op = ops.stiffness_operator(c["P"], _td(c["D"]), c["dtype"])
    bufs, out = _guarded(c, ("y",))
    op(_td(c["x"]), _rows(c, None, "cc", ncells), out["y"], _rows(c, None, "G", ncells), _rows(c, None, "dofmap", ncells))
    results = _collect(c, bufs, out)
    assert lib.get_tuning(lib.TUNE_STIFFNESS_VARIANT) == (1 if target == 128 else 0) and lib.get_tuning(lib.TUNE_XCD_REMAP) == remap
    assert len(ops._PLANS._plans) == 0 and not ops._USE_PLAN, "a plan was built: the launch did not take the column kernel"
    return results


class _MassPlan:
    """A batch plan of ``c``'s entities built through the C ABI with an explicit ``epb``; ``order``: the plan's own entity order;
    ``excl``: with exclusive-dof marks (nothing else adds into y).  ``apply`` launches ``fus_mass_apply_planned_*`` once on ``y``."""

    def __init__(self, lib, c, epb, order=None, excl=False, nent=None):
        import torch

        self.lib, self.L, self.c, self.epb = lib, lib.load(), c, int(epb)
        self.nent, self.N = c["dofmap"].shape[0] if nent is None else nent, c["dofmap"].shape[1]
        self.dm, self.detJ, self.cc, self.x = _td(c["dofmap"]), _td(c["detJ"]), _td(c["cc"]), _td(c["x"])
        assert int(self.dm.max().item()) < c["ndofs"] and int(self.dm.min().item()) >= 0 and self.N * self.epb <= ob.PLAN_MAX_ENTRIES
        self.order = None if order is None else _td(np.asarray(order, dtype=np.int32))
        nbytes = int(self.L.fus_plan_bytes(self.N, self.epb, self.nent))
        assert nbytes > 0
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        lib.check(self.L.fus_plan_build_ordered(self.dm.data_ptr(), None if self.order is None else self.order.data_ptr(), self.N, self.epb,
                                                self.nent, self.ws.data_ptr(), nbytes, lib.stream_ptr()), "fus_plan_build_ordered")
        if excl:
            use = torch.zeros(c["ndofs"], dtype=torch.int32, device="cuda")
            lib.check(self.L.fus_plan_mark_exclusive(self.ws.data_ptr(), self.N, self.epb, self.nent, use.data_ptr(), c["ndofs"], lib.stream_ptr()),
                      "fus_plan_mark_exclusive")
            torch.cuda.synchronize()

    def apply(self, y):
        fn = getattr(self.L, "fus_mass_apply_planned_" + ("f64" if self.c["dtype"] == np.float64 else "f32"))
        self.lib.check(fn(self.x.data_ptr(), self.cc.data_ptr(), y.data_ptr(), self.detJ.data_ptr(), self.ws.data_ptr(), self.N, self.epb,
                          self.nent, self.lib.stream_ptr()), "fus_mass_apply_planned")

    def release(self):
        import torch

        torch.cuda.synchronize()
        self.L.fus_plan_release(self.ws.data_ptr())


def _mass_planned(lib, c, epb, what, order=None, excl=False, runs=None):
    """Build, (mark,) launch, check; with marks a second launch on the same y must give y0 + 2 add.  -> the plan's encoding."""
    if runs is not None:
        lib.set_tuning(lib.TUNE_PLAN_RUNS, 2 if runs else 0)
    plan = _MassPlan(lib, c, epb, order, excl)
    try:
        bufs, out = _guarded(c, ("y",))
        plan.apply(out["y"])
        results = _collect(c, bufs, out)
        enc = _encoding(lib, plan.ws, c["dtype"])
        nbatch = -(-plan.nent // plan.epb)
        if runs is not None:
            assert lib.get_tuning(lib.TUNE_PLAN_RUNS) == (2 if runs else 0)
            assert enc[0] == nbatch and enc[2] == bool(runs) and (0 <= enc[1] <= nbatch if runs else enc[1] == 0), f"{what}: encoding {enc}"
        _check_apply(c, results, what + f" [{enc[1]} of {enc[0]} batches run-coded]")
        if excl:
            plan.apply(out["y"])
            (got, guard), = _collect(c, bufs, out).values()
            rec = c["out"]["y"]
            assert guard
            _check(got, rec, what + " second launch", ref=rec["y0"].astype(np.float64) + 2.0 * rec["add"])
    finally:
        plan.release()
    return enc


def _mass_free(lib, c, nent=None):
    """One launch of ``fus_mass_apply_*`` (mass_kernel) on the dofmap itself."""
    nent, N = c["dofmap"].shape[0] if nent is None else nent, c["dofmap"].shape[1]
    dm, detJ, cc, x = _td(c["dofmap"]), _td(c["detJ"]), _td(c["cc"]), _td(c["x"])
    assert nent == 0 or (int(dm.max().item()) < c["ndofs"] and int(dm.min().item()) >= 0)
    bufs, out = _guarded(c, ("y",))
    fn = getattr(lib.load(), "fus_mass_apply_" + ("f64" if c["dtype"] == np.float64 else "f32"))
    lib.check(fn(x.data_ptr(), cc.data_ptr(), out["y"].data_ptr(), detJ.data_ptr(), dm.data_ptr(), N, nent, lib.stream_ptr()), "fus_mass_apply")
    return _collect(c, bufs, out)


# ---- (a) the build matrix --------------------------------------------------------------------------------------------------------------
GRADIENT = ob.of_family("gradient")


@pytest.mark.parametrize("b", GRADIENT, ids=[ob.case_id(b) for b in GRADIENT])
def test_every_gradient_build_matches_the_fp64_model(gpu, b):
    """Steered as the in-kernel-geometry stiffness kernel is in tests/test_cell_builds_gpu.py, on its shapes.  ORDERED: the cells are
    handed over as "the even ones, then the odd ones", an order the plan cache replaces by one of its own.  RUNS: ``TUNE_PLAN_RUNS`` 2
    makes every launch read the run tables, 0 builds the plan without them.  ONEACC follows from the type and the degree."""
    ops, lib = gpu
    f = dict(b.flags)
    c = _box_case("gradient", b.P, SHAPES[b.P], DTYPES[b.dtype])
    nc, cpb = c["ncells"], lib.load().fus_plan_entities_per_batch((b.P + 1) ** 3)
    assert cpb == ob.cells_per_batch(b.P) and 2 * cpb < nc <= 4 * cpb and nc % cpb != 0
    rows = np.concatenate((np.arange(0, nc, 2), np.arange(1, nc, 2))) if f["ordered"] else None
    lib.set_tuning(lib.TUNE_PLAN_RUNS, 2 if f["runs"] else 0)
    results = _gradient(ops, c, rows)
    assert (ops._PLANS.last_order is not None) == f["ordered"], "the plan cache did not keep the intended cell order"
    (ws, *_), = ops._PLANS._plans.values()
    nbatch, with_runs, reads = _encoding(lib, ws, c["dtype"])
    assert lib.get_tuning(lib.TUNE_PLAN_RUNS) == (2 if f["runs"] else 0) and nbatch == -(-nc // cpb)
    assert (with_runs, reads) == ((nbatch, True) if f["runs"] else (0, False)), f"{with_runs} of {nbatch} batches carry a run table, read: {reads}"
    _check_apply(c, results, ob.case_id(b) + (" ONEACC" if ob.template_key(b)[2][3] else " three accumulators"))


COL = [(b, remap) for b in ob.of_family("col") for remap in (0, 1)]


@pytest.mark.parametrize("b,remap", COL, ids=[f"{ob.case_id(b)}-remap{r}" for b, r in COL])
def test_every_column_build_matches_the_fp64_model(gpu, b, remap):
    """``ops.use_plan(False)``; ``TUNE_STIFFNESS_VARIANT`` 0 / 1 picks ~256 / ~128 threads, ``TUNE_XCD_REMAP`` the block placement.  At
    least 9 workgroups, never a multiple of 8 (both sides of ``xcd < rem``), a partial last workgroup where CPB > 1."""
    ops, lib = gpu
    target = dict(b.flags)["target"]
    shape = ob.COL_SHAPES[b.P, target]
    c = _box_case("general", b.P, shape, DTYPES[b.dtype])
    cpb = ob.default_cells_per_block(b.P, target)
    nb = -(-c["ncells"] // cpb)
    assert nb >= 9 and nb % 8 != 0 and (cpb == 1 or c["ncells"] % cpb != 0)
    _check_apply(c, _col(ops, lib, c, target, remap), f"{ob.case_id(b)}-remap{remap} {nb} workgroups of {cpb} cells")


MASS_PLAN = ob.of_family("mass_plan")


def _mass_shape_case(s, dtype):
    return _box_case("mass", s.P, s.box, dtype) if s.entity == "cell" else _facet_case(s.P, s.box, dtype)


@pytest.mark.parametrize("b", MASS_PLAN, ids=[ob.case_id(b) for b in MASS_PLAN])
def test_every_planned_mass_build_matches_the_fp64_model(gpu, b):
    """Through the C ABI with an explicit (N, epb): the two shapes of the build's bucket (its lowest ept; its largest N x epb), each
    with ``TUNE_PLAN_RUNS`` 0 and 2 and with the natural and a permuted entity order.  At least three batches, the last one ragged.
    With marks a second launch on the same y gives y0 + 2 add."""
    ops, lib = gpu
    f = dict(b.flags)
    bucket = ob.template_key(b)[2][0]
    for s in ob.MASS_PLAN_SHAPES[bucket]:
        c = _mass_shape_case(s, DTYPES[b.dtype])
        nent, N = c["dofmap"].shape
        assert (N, s.epb) in f["shapes"] and nent == ob.mass_shape_entities(s) > 2 * s.epb and nent % s.epb != 0
        assert ob.mass_plan_ept(N, s.epb)[1] == bucket
        perm = np.random.default_rng(nent).permutation(nent)
        for runs in (False, True):
            for order in (None, perm):
                what = (f"{ob.case_id(b)} {s.entity} N={N} epb={s.epb} ept={ob.mass_plan_ept(N, s.epb)[0]} {nent} entities "
                        f"{'runs' if runs else 'lists'} {'natural' if order is None else 'permuted'}")
                _mass_planned(lib, c, s.epb, what, order, f["excl"], runs)


PYTHON_ROUTE = [(entity, P, d) for entity in ("cell", "facet") for P in ob.DEGREES for d in DTYPES]


@pytest.mark.parametrize("entity,P,dtype", PYTHON_ROUTE, ids=[f"{e}-P{P}-{d}" for e, P, d in PYTHON_ROUTE])
def test_the_python_route_to_the_planned_mass_kernel(gpu, entity, P, dtype):
    """``mass_operator(N, T, atomic=True)`` without and with ``exclusive=True`` on the smallest sets that take the planned route:
    ``mass_kernel_name`` says so, and the batch size the library picks falls into the bucket tests/cell_op_builds.py names."""
    ops, lib = gpu
    if entity == "cell":
        c, want = _box_case("mass", P, ob.MASS_CELL_BOXES[P], DTYPES[dtype]), ob.MASS_CELL_EPT[P]
    else:
        c, want = _facet_case(P, ob.mass_facet_box(P), DTYPES[dtype]), 4 if P == 7 else 5
    nent, N = c["dofmap"].shape
    epb = lib.load().fus_plan_entities_per_batch(N)
    assert epb == ob.entities_per_batch(N) and ob.mass_plan_ept(N, epb)[1] == want and nent * N >= ob.MASS_MIN_ENTRIES == ops._MASS_PLAN_MIN_ENTRIES
    dm = _td(c["dofmap"])
    assert ops.mass_kernel_name(dm, c["ndofs"], atomic=True) == "fus::mass_plan_kernel"
    for excl in (False, True):
        bufs, out = _guarded(c, ("y",))
        ops.mass_operator(N, c["dtype"], exclusive=excl, atomic=True)(_td(c["x"]), _td(c["cc"]), out["y"], _td(c["detJ"]), dm)
        _check_apply(c, _collect(c, bufs, out), f"python {entity} P={P} {dtype} N={N} epb={epb} EPT={want} {'marks' if excl else 'atomics'}")
        assert len(ops._PLANS._plans) == 1 + excl


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("what", ["cells", "facets", "N1"])
def test_the_32_bit_mass_kernel_on_small_sets(gpu, what, dtype):
    """Cells (P = 4), boundary facets (P = 3) and entities of one dof each: a few workgroups, the last one partly idle."""
    ops, lib = gpu
    T = DTYPES[dtype]
    c = {"cells": lambda: _box_case("mass", 4, SHAPES[4], T), "facets": lambda: _facet_case(3, (3, 3, 2), T),
         "N1": lambda: _case("mass", ("N1", dtype), lambda: model.entities(T, 1, 1003, 301))}[what]()
    assert c["dofmap"].size % 256 != 0 and ob.mass_index_type(c["dofmap"].size) == "unsigned int"
    _check_apply(c, _mass_free(lib, c), f"mass_kernel u32 {what} {dtype} N={c['dofmap'].shape[1]}")


MASS = {ob.case_id(b): b for b in ob.of_family("mass")}


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_mass_kernel_takes_a_second_trip(gpu, dtype):
    """Just over 256 x 64 x 256 entries of a colliding synthetic dofmap: the grid is at its cap and the first threads take a second
    trip of the grid-stride loop.  The model's ``add`` is ``np.add.at`` in fp64."""
    ops, lib = gpu
    b = MASS[f"mass-{dtype}-u32"]
    st = ob.MASS_SECOND_TRIP
    c = _case("mass", ("second trip", dtype), lambda: model.entities(DTYPES[dtype], st["N"], st["nent"], st["ndofs"]))
    total = c["dofmap"].size
    assert total == dict(b.flags)["total"] and ob.MASS_GRID_ENTRIES < total < ob.MASS_GRID_ENTRIES + 256 * 64
    plain = np.zeros(c["ndofs"])
    w = c["detJ"].astype(np.float64) * c["cc"].astype(np.float64)[:, None]
    np.add.at(plain, c["dofmap"].reshape(-1), (c["x"].astype(np.float64)[c["dofmap"]] * w).reshape(-1))
    assert rel_max(c["out"]["y"]["add"], plain) < 1e-13
    _check_apply(c, _mass_free(lib, c), f"{ob.case_id(b)} second trip, {total} entries")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_64_bit_mass_kernel_at_2_31_entries(gpu, dtype):
    """N = 2048, 2^20 entities: 2^31 entries, the smallest size that takes the 64-bit build.  Built on the device with positive inputs;
    entry i goes to dof i mod ndofs (ndofs = 2^20 - 3), so the fp64 reference of a range of entries is a sum over the rows of a
    [rows, ndofs] view, computed in chunks.  The last 4096 entities carry constants 64 times larger: what they add is about a fifth of
    every dof's sum.  Checks: the whole launch equals the sum of two half launches (2^30 entries each: the 32-bit build that the small
    cases pin); the whole launch equals the fp64 reference, and so do the last 4096 entities alone, taken as the difference of the whole
    launch and a launch without them in fp64 arithmetic on the host.  The only case that takes more than a few seconds; it prints its time."""
    import torch

    ops, lib = gpu
    b = MASS[f"mass-{dtype}-i64"]
    big = ob.MASS_BIG
    N, nent, ndofs = big["N"], big["nent"], big["ndofs"]
    total = N * nent
    assert total == dict(b.flags)["total"] == 2**31 and ob.mass_index_type(total) == "long" and ob.mass_index_type(total // 2) == "unsigned int"
    tdt = torch.float64 if dtype == "f64" else torch.float32
    need = total * (4 + tdt.itemsize) + (6 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need / 2**30:.0f} GiB of free device memory, {free / 2**30:.0f} GiB are free")
    t0 = time.perf_counter()
    d = torch.device("cuda", 0)
    gen = torch.Generator(device=d).manual_seed(31)
    CH = 1 << 26  # entries per chunk
    dm = torch.empty(total, dtype=torch.int32, device=d)
    detJ = torch.empty(total, dtype=tdt, device=d)
    for a in range(0, total, CH):
        dm[a:a + CH] = (torch.arange(a, a + CH, device=d, dtype=torch.int64) % ndofs).to(torch.int32)
        detJ[a:a + CH] = 0.5 + torch.rand(CH, dtype=tdt, device=d, generator=gen)
    ntail = 4096
    cc = 0.75 + 0.5 * torch.rand(nent, dtype=tdt, device=d, generator=gen)
    cc[nent - ntail:] *= 64.0
    x = 0.5 + torch.rand(ndofs, dtype=tdt, device=d, generator=gen)
    assert int(dm[-1].item()) == (total - 1) % ndofs and int(dm.max().item()) == ndofs - 1 and int(dm.min().item()) == 0

    def reference(e0, e1):
        """sum over the entries of the entities [e0, e1) per dof, in fp64: entry i sits in column i mod ndofs."""
        ref = torch.zeros(ndofs, dtype=torch.float64, device=d)
        a, end = e0 * N, e1 * N
        while a < end:
            z = min(end, a + CH)
            w = detJ[a:z].double() * cc[a // N:(z + N - 1) // N].double().repeat_interleave(N)[a % N:a % N + (z - a)]
            head = min((-a) % ndofs, z - a)  # up to the next multiple of ndofs
            ref[a % ndofs:a % ndofs + head] += w[:head]
            rows = (z - a - head) // ndofs
            ref += w[head:head + rows * ndofs].view(rows, ndofs).sum(dim=0)
            rest = z - a - head - rows * ndofs
            ref[:rest] += w[head + rows * ndofs:]
            a = z
        return ref * x.double()

    fn = getattr(lib.load(), "fus_mass_apply_" + dtype)
    size = tdt.itemsize

    def launch(e0, e1):
        buf = torch.full((ndofs + GUARD,), SENTINEL, dtype=tdt, device=d)
        y = buf[:ndofs]
        y.zero_()
        lib.check(fn(x.data_ptr(), cc.data_ptr() + e0 * size, y.data_ptr(), detJ.data_ptr() + e0 * N * size, dm.data_ptr() + e0 * N * 4, N,
                     e1 - e0, lib.stream_ptr()), "fus_mass_apply")
        torch.cuda.synchronize()
        assert bool((buf[ndofs:] == SENTINEL).all().item()), "the launch wrote behind y"
        return y.double()

    t1 = time.perf_counter()
    whole = launch(0, nent)
    t2 = time.perf_counter()
    halves = launch(0, nent // 2) + launch(nent // 2, nent)
    ref = reference(0, nent)
    tol = TOL[np.dtype(DTYPES[dtype])]
    rl2 = lambda a, r: float(((a - r).norm() / r.norm()).item())  # noqa: E731
    rmx = lambda a, r: float(((a - r).abs().max() / r.abs().max()).item())  # noqa: E731
    figures = dict(halves=(rl2(whole, halves), rmx(whole, halves)), model=(rl2(whole, ref), rmx(whole, ref)))
    tail_ref = reference(nent - ntail, nent)
    tail = whole - launch(0, nent - ntail)
    assert float((tail_ref / ref).min().item()) > 0.05  # the tail is a sizeable part of every dof's sum
    # the difference of two fp32 sums of ~2000 carries both sums' rounding: measured against the size of the sums, as TOL is
    figures["tail"] = (float(((tail - tail_ref).norm() / ref.norm()).item()), float(((tail - tail_ref).abs().max() / ref.abs().max()).item()))
    t3 = time.perf_counter()
    print(f"{ob.case_id(b)}: 2^31 entries on {ndofs} dofs; " + "; ".join(f"{k} l2 {v[0]:.3e} max {v[1]:.3e}" for k, v in figures.items()) +
          f"; set-up {t1 - t0:.1f} s, the launch with its synchronisation {t2 - t1:.2f} s, the case {t3 - t0:.1f} s")
    for k, (e2, em) in figures.items():
        assert e2 < tol["l2"] and em < tol["mx"], (k, e2, em)


# ---- (b) edge cases --------------------------------------------------------------------------------------------------------------------
FAMILIES = ("gradient", "col256", "col128", "mass_plan", "mass_plan_excl", "mass")
KIND = {"gradient": "gradient", "col256": "general", "col128": "general", "mass_plan": "mass", "mass_plan_excl": "mass", "mass": "mass"}


def _edge_cases(degrees):
    return [(fam, d, P) for P in degrees for d in DTYPES for fam in FAMILIES]


def _edge_id(e):
    return f"{e[0]}-P{e[2]}-{e[1]}"


def _edge(gpu, e, c, what, ncells=None):
    """One launch of family ``e[0]`` on the first ``ncells`` cells of ``c`` (all of them by default) at the library's defaults."""
    ops, lib = gpu
    fam = e[0]
    if fam == "gradient":
        return _gradient(ops, c, None, ncells)
    if fam.startswith("col"):
        return _col(ops, lib, c, int(fam[3:]), 0, ncells)
    if fam == "mass":
        return _mass_free(lib, c, ncells)
    epb = lib.load().fus_plan_entities_per_batch(c["dofmap"].shape[1])
    _mass_planned(lib, c, epb, f"{_edge_id(e)} {what}", None, fam.endswith("excl"))
    return None  # (checked inside)


ONE_CELL = _edge_cases((1, 4, 10))


@pytest.mark.parametrize("e", ONE_CELL, ids=[_edge_id(e) for e in ONE_CELL])
def test_one_cell(gpu, e):
    """One cell: one batch or workgroup with 63 of 64 (P = 1), 9 of 10 (P = 4), 1 of 2 (P = 10) cell slots idle."""
    c = _box_case(KIND[e[0]], e[2], (1, 1, 1), DTYPES[e[1]])
    assert c["ncells"] == 1
    results = _edge(gpu, e, c, "one cell")
    if results is not None:
        _check_apply(c, results, f"{_edge_id(e)} one cell")


ZERO_CELLS = _edge_cases((4,))


@pytest.mark.parametrize("e", ZERO_CELLS, ids=[_edge_id(e) for e in ZERO_CELLS])
def test_zero_cells(gpu, e):
    """An empty cell range: nothing is raised, nothing is launched, every output is unchanged to the bit, no plan is cached."""
    ops, lib = gpu
    c = _box_case(KIND[e[0]], e[2], (1, 1, 1), DTYPES[e[1]])
    if e[0].startswith("mass_plan"):  # the C ABI with a plan of the one cell and nent = 0
        plan = _MassPlan(lib, c, lib.load().fus_plan_entities_per_batch(c["dofmap"].shape[1]))
        try:
            plan.nent = 0
            bufs, out = _guarded(c, ("y",))
            plan.apply(out["y"])
            results = _collect(c, bufs, out)
        finally:
            plan.release()
    else:
        results = _edge(gpu, e, c, "no cell", ncells=0)
    for k, (got, guard) in results.items():
        assert guard and np.array_equal(got, c["out"][k]["y0"]), k
    assert len(ops._PLANS._plans) == 0


FULL_BATCH = [(e, shape) for P, shape in ((4, (5, 2, 2)), (7, (3, 2, 2))) for e in _edge_cases((P,))]


@pytest.mark.parametrize("e,shape", FULL_BATCH, ids=[_edge_id(e) for e, _ in FULL_BATCH])
def test_exactly_full_last_batch(gpu, e, shape):
    """P = 4: 20 cells in two batches of 10 (four workgroups of 5 at ~128 threads); P = 7: 12 cells in three batches of 4 (six of 2)."""
    c = _box_case(KIND[e[0]], e[2], shape, DTYPES[e[1]])
    cpb = ob.default_cells_per_block(e[2], 128 if e[0] == "col128" else 256)
    assert c["ncells"] % cpb == 0 and c["ncells"] > cpb
    what = f"{c['ncells']} cells in full batches of {cpb}"
    results = _edge(gpu, e, c, what)
    if results is not None:
        _check_apply(c, results, f"{_edge_id(e)} {what}")


COLLIDING = _edge_cases((3,))


@pytest.mark.parametrize("e", COLLIDING, ids=[_edge_id(e) for e in COLLIDING])
def test_colliding_dofmap(gpu, e):
    """Scatter-add under heavy collisions: P = 3, 37 cells whose dofmap rows are random integers in [0, 50) -- dofs repeat inside a cell
    and every batch touches every dof (with marks: no dof is exclusive to a batch); the geometry is a tiled 2 x 2 x 2 mesh."""
    c = _colliding_case(KIND[e[0]], DTYPES[e[1]])
    assert c["ncells"] == 37 and c["ndofs"] == 50 and c["dofmap"].max() < 50
    results = _edge(gpu, e, c, "colliding dofmap")
    if results is not None:
        _check_apply(c, results, f"{_edge_id(e)} colliding dofmap")
