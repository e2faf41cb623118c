"""The general-G planned apply that reads one slot per local ROW and the compact run tables (csrc/stiffness_plan.hpp:
``stiffness_plan_rows_kernel``; layout: csrc/plan.hpp ``rowbase`` / ``runs_c``; knob ``TUNE_PLAN_ROWS``).

What can go wrong is where a thread learns its slot, so the shapes are the smallest at which that differs: rows of cells straddled by
batches, a ragged last batch, more than one batch, the three LDS builds (P = 2: own buffers, P = 4: aliased with the whole G slab,
P = 6: aliased with a ring).  Reference and tolerance: ``oracle_c.stiffness_apply`` and the ``_check`` rule of test_operators_gpu.py
(fp64: rel l2 < 1e-12, rel max < 1e-11), K 1 = 0 to that file's bound (max |K 1| < 1e-10 max |K u|)."""
import numpy as np
import pytest

from conftest import TOL, build_problem, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

K_PLAN_MAX_RUNS = 128
SHAPES = [(4, (3, 2, 7)), (2, (3, 3, 5)), (6, (2, 2, 3))]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    torch.cuda.set_device(0)
    return pkg("device"), pkg("operators")


@pytest.fixture(autouse=True)
def _fresh_plans(gpu):
    _, ops = gpu
    lib = pkg("_lib")
    ops._PLANS.clear()
    ops.use_plan(True)
    yield
    lib.set_tuning(lib.TUNE_PLAN_ROWS, 1)
    ops._PLANS.clear()


@pytest.fixture(scope="module")
def problems():
    """one problem per shape, built once and left unchanged"""
    return {(P, cells): build_problem(P, cells, perturb=0.16, seed=11) for P, cells in SHAPES}


def _check(got, ref, dtype, what):
    tol = TOL[np.dtype(dtype)]
    e2, em = rel_l2(got, ref), rel_max(got, ref)
    assert e2 < tol["l2"] and em < tol["mx"], f"{what}: rel l2 {e2:.3e} (tol {tol['l2']}), rel max {em:.3e}"


def _align256(v):
    return (v + 255) // 256 * 256


def _layout(N, epb, nent):
    """byte offsets of the regions of a cell plan (csrc/plan.hpp: plan_view_generic); everything up to ``order`` is where it has always been,
    and ``excl`` is still the last region"""
    nbatch, M, n = -(-nent // epb), epb * N, round(N ** (1 / 3))
    off, out = 256, {"nbatch": nbatch, "M": M}
    for name, size in (("nu", nbatch * 4), ("udofs", nbatch * M * 4), ("runs", nbatch * 2 * K_PLAN_MAX_RUNS * 4), ("slot", nbatch * M * 2),
                       ("order", nent * 4), ("rowbase", nbatch * (M // n) * 2), ("runs_c", nbatch * 2 * K_PLAN_MAX_RUNS * 4),
                       ("excl", nbatch * ((M + 31) // 32) * 4)):
        out[name] = off
        off += _align256(size)
    out["bytes"] = off
    return out


def _the_plan(ops):
    """(workspace bytes on the host, entities per batch) of the batch plan built last (every apply of these tests uploads its dofmap
    anew, and the cache keys on the array's identity: one entry per apply, all of the same dofmap)"""
    ws, _, epb = [v for k, v in ops._PLANS._plans.items() if k[-1] != "strips"][-1]
    return ws.cpu().numpy(), epb


def _header(ws):
    """(rows_consecutive, run_stride) of a plan's header"""
    h = ws[:256].view(np.int64)
    return int(h[8]), int(h[9])


def _expected(dofmap, epb, order=None):
    """From the dofmap alone: (every row consecutive, run_stride, slots per batch) as the layout defines them"""
    nent, N = dofmap.shape
    n = round(N ** (1 / 3))
    dm = dofmap if order is None else dofmap[order]
    rows = dm.reshape(nent, N // n, n).astype(np.int64)
    consecutive = bool((rows == rows[:, :, :1] + np.arange(n)).all())
    most, slots = 0, []
    for b in range(0, nent, epb):
        ent = dm[b:b + epb].ravel()
        u = np.unique(ent)
        nr = 1 + int((np.diff(u) != 1).sum())
        most = max(most, nr if (nr <= K_PLAN_MAX_RUNS and 2 * nr < u.size) else K_PLAN_MAX_RUNS)
        slots.append(np.searchsorted(u, ent).astype(np.uint16))
    stride = 1
    while stride < most:
        stride *= 2
    return consecutive, stride, slots


def _stiffness(gpu, pb, dofmap, x, G=None, cc=None):
    dev, ops = gpu
    y = dev.to_device(np.zeros(x.shape[0]))
    ops.stiffness_operator(pb["P"], pb["D"].flatten(), np.float64)(
        dev.to_device(x), dev.to_device(pb["cc"] if cc is None else cc), y, dev.to_device(pb["G"] if G is None else G),
        dev.to_device(np.ascontiguousarray(dofmap)))
    return y.copy_to_host()


def _mass_and_geometry(gpu, oracle_c, pb, dofmap, x, y_ref, what):
    """the other readers of the same workspace (its ``slot`` region): the planned cell mass and the in-kernel-geometry stiffness"""
    dev, ops = gpu
    mesh, P = pb["mesh"], pb["P"]
    dm = dev.to_device(np.ascontiguousarray(dofmap))
    y = dev.to_device(np.zeros(mesh.ndofs))
    ops.stiffness_operator(P, pb["D"].flatten(), np.float64, geometry=(mesh.x_dofs, mesh.x_g, pb["pts"], pb["wts"]))(
        dev.to_device(x), dev.to_device(pb["cc"]), y, None, dm)
    _check(y.copy_to_host(), y_ref, np.float64, f"in-kernel geometry, {what}")
    m_ref = np.zeros(mesh.ndofs)
    oracle_c.mass_apply(x, pb["cc"], m_ref, pb["detJ"], np.ascontiguousarray(dofmap))
    y = dev.to_device(np.zeros(mesh.ndofs))
    old_min, ops._MASS_PLAN_MIN_ENTRIES = ops._MASS_PLAN_MIN_ENTRIES, 1
    try:
        ops.mass_operator((P + 1) ** 3, np.float64)(dev.to_device(x), dev.to_device(pb["cc"]), y, dev.to_device(pb["detJ"]), dm)
    finally:
        ops._MASS_PLAN_MIN_ENTRIES = old_min
    _check(y.copy_to_host(), m_ref, np.float64, f"planned mass, {what}")


@pytest.mark.parametrize("P,cells", SHAPES, ids=[f"P{P}" for P, _ in SHAPES])
def test_box_mesh_plan_takes_the_rows_kernel(gpu, oracle_c, problems, P, cells):
    dev, ops = gpu
    lib = pkg("_lib")
    pb = problems[(P, cells)]
    mesh = pb["mesh"]
    assert lib.get_tuning(lib.TUNE_PLAN_ROWS) == 1, "the default is auto"
    y_ref = np.zeros(mesh.ndofs)
    oracle_c.stiffness_apply(P, pb["D"], pb["x"], pb["cc"], y_ref, pb["G"], mesh.dofmap)
    for knob in (1, 0):
        lib.set_tuning(lib.TUNE_PLAN_ROWS, knob)
        assert lib.get_tuning(lib.TUNE_PLAN_ROWS) == knob
        _check(_stiffness(gpu, pb, mesh.dofmap, pb["x"]), y_ref, np.float64, f"P={P} {cells}, rows knob {knob}")
    ws, epb = _the_plan(ops)
    lay = _layout((P + 1) ** 3, epb, mesh.ncells)
    assert ws.size == lay["bytes"]
    consecutive, stride, _ = _expected(mesh.dofmap, epb, None if ops._PLANS.last_order is None else ops._PLANS.last_order.cpu().numpy())
    assert consecutive, "a box-mesh dofmap has consecutive rows"
    assert _header(ws) == (1, stride)
    if P == 4:
        assert lay["nbatch"] == 5 and stride == 64  # up to 47 runs per batch
    # the compact table is the full one at the smaller stride
    full = ws[lay["runs"]:lay["runs"] + lay["nbatch"] * 1024].view(np.int32).reshape(lay["nbatch"], 2 * K_PLAN_MAX_RUNS)
    compact = ws[lay["runs_c"]:lay["runs_c"] + lay["nbatch"] * 8 * stride].view(np.int32).reshape(lay["nbatch"], 2 * stride)
    assert (compact == full[:, :2 * stride]).all()
    # K 1 = 0 with the rows kernel
    lib.set_tuning(lib.TUNE_PLAN_ROWS, 1)
    K1 = _stiffness(gpu, pb, mesh.dofmap, np.ones(mesh.ndofs))
    assert np.abs(K1).max() < 1e-10 * np.abs(y_ref).max()
    _mass_and_geometry(gpu, oracle_c, pb, mesh.dofmap, pb["x"], y_ref, f"P={P}")


def _renumbered(pb, perm):
    """the problem in the numbering new = perm[old]: (dofmap, x)"""
    x = np.empty_like(pb["x"])
    x[perm] = pb["x"]
    return np.ascontiguousarray(perm[pb["mesh"].dofmap]), x


def test_random_renumbering_keeps_the_slot_kernel(gpu, oracle_c, problems):
    dev, ops = gpu
    P, cells = SHAPES[0]
    pb = problems[(P, cells)]
    mesh = pb["mesh"]
    perm = np.random.default_rng(3).permutation(mesh.ndofs).astype(mesh.dofmap.dtype)
    dofmap, x = _renumbered(pb, perm)
    y_ref = np.zeros(mesh.ndofs)
    oracle_c.stiffness_apply(P, pb["D"], x, pb["cc"], y_ref, pb["G"], dofmap)
    _check(_stiffness(gpu, pb, dofmap, x), y_ref, np.float64, "random renumbering")
    ws, epb = _the_plan(ops)
    lay = _layout((P + 1) ** 3, epb, mesh.ncells)
    order = None if ops._PLANS.last_order is None else ops._PLANS.last_order.cpu().numpy()
    consecutive, _, slots = _expected(dofmap, epb, order)
    assert not consecutive
    assert _header(ws)[0] == 0
    # the slot region: where it always was, holding what it always held (the position of each entry's dof among the batch's sorted dofs)
    for b, s in enumerate(slots):
        got = ws[lay["slot"] + 2 * b * lay["M"]:lay["slot"] + 2 * b * lay["M"] + 2 * s.size].view(np.uint16)
        assert got.tobytes() == s.tobytes(), f"slots of batch {b}"
    _mass_and_geometry(gpu, oracle_c, pb, dofmap, x, y_ref, "random renumbering")


def test_one_broken_row_switches_the_whole_plan(gpu, oracle_c, problems):
    dev, ops = gpu
    P, cells = SHAPES[0]
    pb = problems[(P, cells)]
    mesh = pb["mesh"]
    n = P + 1
    # two neighbouring dofs of an interior row (ix = 1, ty = 1) of one cell in the middle of the mesh, swapped everywhere
    c = mesh.ncells // 2
    a, b = (int(v) for v in mesh.dofmap[c, n * n + n + 1:n * n + n + 3])
    assert b == a + 1 and (mesh.dofmap == a).sum() == 1 and (mesh.dofmap == b).sum() == 1
    perm = np.arange(mesh.ndofs, dtype=mesh.dofmap.dtype)
    perm[a], perm[b] = b, a
    dofmap, x = _renumbered(pb, perm)
    y_ref = np.zeros(mesh.ndofs)
    oracle_c.stiffness_apply(P, pb["D"], x, pb["cc"], y_ref, pb["G"], dofmap)
    _check(_stiffness(gpu, pb, dofmap, x), y_ref, np.float64, "one broken row")
    ws, epb = _the_plan(ops)
    rows = dofmap.reshape(mesh.ncells, n * n, n).astype(np.int64)
    assert int((rows != rows[:, :, :1] + np.arange(n)).any(axis=2).sum()) == 1, "exactly one row of one cell is broken"
    assert _header(ws)[0] == 0, "one broken row: the plan as a whole keeps the slot kernel"


def test_shuffled_cells_take_the_ordered_rows_kernel(gpu, oracle_c, problems):
    dev, ops = gpu
    P, cells = SHAPES[0]
    pb = problems[(P, cells)]
    mesh = pb["mesh"]
    perm = np.random.default_rng(3).permutation(mesh.ncells)
    dm, G, cc = (np.ascontiguousarray(a[perm]) for a in (mesh.dofmap, pb["G"], pb["cc"]))
    y_ref = np.zeros(mesh.ndofs)
    oracle_c.stiffness_apply(P, pb["D"], pb["x"], cc, y_ref, G, dm)
    _check(_stiffness(gpu, pb, dm, pb["x"], G=G, cc=cc), y_ref, np.float64, "shuffled cells, ordered plan")
    assert ops._PLANS.last_order is not None, "the random order must have triggered the locality plan"
    ws, epb = _the_plan(ops)
    consecutive, stride, _ = _expected(dm, epb, ops._PLANS.last_order.cpu().numpy())
    assert consecutive and _header(ws) == (1, stride)
