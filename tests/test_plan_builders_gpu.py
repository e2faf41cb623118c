"""The two plan builders on the device (csrc/plan_build.hpp, csrc/mass_gather.hpp) against the index model of tests/plan_model.py, byte
for byte: every region of the batch plan, the exclusive-dof marks, the transposed gather plan and its static companion.

Protocol of every build: a buffer of ``bytes`` + 256 filled with 0xA5; the size is the one the library reports; after the build every
DEFINED byte equals the model's, every byte the builder must not touch (alignment gaps, the tail of a ragged batch, regions the call
does not fill, the 256 guard bytes) still holds 0xA5.  The shapes are the smallest that take each path: every build of the sort kernel
at both edges of its range, every cell degree, both sides of the run rule, the second iteration of the two grid-stride loops, the block
edges of the gather plan.  No number in this file is a tolerance."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import plan_model as pm
from conftest import pkg

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    torch.cuda.set_device(0)
    return pkg("_lib"), pkg("_lib").load()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


@contextlib.contextmanager
def _workspace(L, nbytes):
    """a device buffer of ``nbytes`` + the guard, all 0xA5; whatever was built in it is forgotten on the way out"""
    import torch

    ws = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    try:
        yield ws
    finally:
        L.fus_plan_release(ws.data_ptr())


def _regions(lay, names, nbatch):
    """(name, first byte, one past its last byte incl. the gap behind it, bytes per batch) of the header and the regions of a layout"""
    offs = sorted((lay[k], k) for k in names)
    out = [("header", 0, offs[0][0] if offs else lay["bytes"], 256)]
    for i, (off, k) in enumerate(offs):
        end = offs[i + 1][0] if i + 1 < len(offs) else lay["bytes"]
        size = lay["size"][k] if "size" in lay else end - off
        out.append((k, off, end, max(1, size // max(1, nbatch))))
    return out


def _assert_image(got, model, regions, what):
    """``got``: the buffer after the build (uint8, guard included); every DEFINED byte as the model's image, every UNTOUCHED one 0xA5"""
    nbytes = model.image.size
    assert got.size == nbytes + GUARD
    assert (got[nbytes:] == FILL).all(), f"{what}: the builder wrote behind the workspace (guard byte {int(np.nonzero(got[nbytes:] != FILL)[0][0])})"
    for name, off, end, per_batch in regions:
        g, want, m = got[off:end], model.image[off:end], model.mask[off:end]
        d = m == pm.DEFINED
        if g[d].tobytes() != want[d].tobytes():
            at = int(np.nonzero(d & (g != want))[0][0])
            pytest.fail(f"{what}: region '{name}' differs from the model, first in batch {at // per_batch} (byte {at} of the region: "
                        f"{int(g[at])} for {int(want[at])}; {int((d & (g != want)).sum())} bytes differ)")
        u = m == pm.UNTOUCHED
        if not (g[u] == FILL).all():
            at = int(np.nonzero(u & (g != FILL))[0][0])
            pytest.fail(f"{what}: region '{name}': byte {at} (batch {at // per_batch}) is not the builder's to write and was written")


def _batch_regions(p):
    return _regions(p.layout, list(p.layout["size"]), p.nbatch)


@contextlib.contextmanager
def _built(L, dofmap, epb, order=None, P=None, allow_runs=True):
    """Builds the batch plan of ``dofmap`` on the device (through fus_stiffness_plan_build if ``P`` is given) and compares it with the
    model; yields (model, workspace)."""
    nent, N = dofmap.shape
    p = pm.batch_plan(dofmap, epb, order=order, allow_runs=allow_runs)
    nbytes = int(L.fus_plan_bytes(N, epb, nent))
    assert nbytes == p.layout["bytes"], f"fus_plan_bytes({N}, {epb}, {nent}) = {nbytes}, the layout gives {p.layout['bytes']}"
    dm_d = _dev(dofmap)
    with _workspace(L, nbytes) as ws:
        if P is not None:
            assert order is None and int(L.fus_stiffness_plan_bytes(P, nent)) == nbytes
            rc = L.fus_stiffness_plan_build(dm_d.data_ptr(), P, nent, ws.data_ptr(), nbytes, None)
        elif order is not None:
            rc = L.fus_plan_build_ordered(dm_d.data_ptr(), _dev(order.astype(np.int32)).data_ptr(), N, epb, nent, ws.data_ptr(), nbytes, None)
        else:
            rc = L.fus_plan_build(dm_d.data_ptr(), N, epb, nent, ws.data_ptr(), nbytes, None)
        assert rc == 0
        _assert_image(_host(ws), p, _batch_regions(p), f"N={N} epb={epb} nent={nent}")
        nb, wr = C.c_int64(-1), C.c_int64(-1)
        assert L.fus_plan_encoding(ws.data_ptr(), C.byref(nb), C.byref(wr), None, None) == 0
        assert (nb.value, wr.value) == (p.nbatch, int(p.use_runs.sum()))
        yield p, ws


def _edge_dofmap(N, epb, pattern):
    return pm.dof_pattern(pattern, N, pm.three_batches(epb), N * epb, seed=N + epb)


# ---- 1: the dispatch on M -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", pm.PATTERNS)
@pytest.mark.parametrize("N,epb", pm.DISPATCH_EDGES, ids=[f"M{N * epb}" for N, epb in pm.DISPATCH_EDGES])
def test_dispatch_edges(gpu, N, epb, pattern):
    """M = 256 ... 4096 and one past each power of two: every build of the sort kernel at both ends of its range, three batches with a
    ragged last one.  ``high``: the largest dof is 2^31 - 2 (the key's dof is unsigned, d + 1 does not wrap)."""
    _, L = gpu
    dm = _edge_dofmap(N, epb, pattern)
    if pattern == "high":
        assert int(dm.max()) == 2 ** 31 - 2
    with _built(L, dm, epb) as (p, _):
        assert p.nbatch == 3 and ((p.nu_count < p.M).any() or epb == 1), "three batches, and the dof list of one at least is padded"
        if pattern != "collide" and pm.plan_row_len(N) > 1:
            assert p.rows_consecutive == 1 and p.use_runs.all()


def test_one_entry_too_many_has_no_plan(gpu):
    _, L = gpu
    assert int(L.fus_plan_bytes(241, 17, 1)) < 0 and 241 * 17 == pm.PLAN_MAX_ENTRIES + 1
    assert int(L.fus_plan_bytes(64, 64, 1)) > 0


# ---- 2: every cell degree -------------------------------------------------------------------------------------------------------

def _box_dofmap(P):
    """the dofmap of a 2 x 2 x k box mesh, k the smallest that gives two batches; where 4 k cells fill their batches exactly, without
    its last cell (the last batch is ragged)"""
    epb = pm.cells_per_batch(P)
    k = epb // 4 + 1
    mesh = pkg("boxmesh").BoxMesh(P, (2, 2, k))
    dm = mesh.dofmap if mesh.ncells % epb else mesh.dofmap[:-1]
    assert dm.shape[0] > epb and dm.shape[0] % epb != 0
    return np.ascontiguousarray(dm), mesh.ndofs


@pytest.mark.parametrize("P", pm.CELL_DEGREES)
def test_every_cell_degree(gpu, P):
    lib, L = gpu
    dm, _ = _box_dofmap(P)
    assert int(L.fus_plan_entities_per_batch((P + 1) ** 3)) == pm.cells_per_batch(P)
    with _built(L, dm, pm.cells_per_batch(P), P=P) as (p, _):
        assert p.rows_consecutive == 1 and p.row_len == P + 1 and p.nbatch >= 2


def _broken_row(dm, ndofs):
    """two neighbouring dofs of an interior row of one cell, swapped everywhere (tests/test_plan_rows_gpu.py)"""
    n = 5
    c = dm.shape[0] // 2
    a, b = (int(v) for v in dm[c, n * n + n + 1:n * n + n + 3])
    assert b == a + 1 and (dm == a).sum() == 1 and (dm == b).sum() == 1
    perm = np.arange(ndofs, dtype=np.int32)
    perm[a], perm[b] = b, a
    return np.ascontiguousarray(perm[dm])


@pytest.mark.parametrize("how", ["one-broken-row", "random-numbering"])
def test_degree_four_without_consecutive_rows(gpu, how):
    _, L = gpu
    dm, ndofs = _box_dofmap(4)
    dm = _broken_row(dm, ndofs) if how == "one-broken-row" else np.ascontiguousarray(np.random.default_rng(3).permutation(ndofs).astype(np.int32)[dm])
    with _built(L, dm, pm.cells_per_batch(4), P=4) as (p, _):
        assert p.rows_consecutive == 0 and p.header[10] == 1
        assert (p.run_stride == 128) == (how == "random-numbering")


# ---- 3: ordered plans -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,epb", pm.ORDERED, ids=[f"{N}x{epb}" for N, epb in pm.ORDERED])
def test_ordered(gpu, N, epb):
    _, L = gpu
    dm = _edge_dofmap(N, epb, "structured")
    order = np.random.default_rng(N).permutation(dm.shape[0]).astype(np.int32)
    with _built(L, dm, epb, order=order) as (p, ws):
        assert p.header[6] == 1 and p.mask[p.layout["order"]:p.layout["order"] + 4 * p.nent].all()
        assert not (p.slot == pm.batch_plan(dm, epb).slot).all(), "the order changes the plan"


# ---- 4: the run rule ------------------------------------------------------------------------------------------------------------

def _runs_of(lengths, gap=3):
    """distinct dofs forming runs of the given lengths"""
    out, d = [], 5
    for n in lengths:
        out.extend(range(d, d + n))
        d += n + gap
    return np.array(out, np.int32)


RUN_RULE = {"128-runs-of-4": ([4] * 128, 128, True), "129-runs": ([4] * 127 + [2, 2], 129, False), "2nr-equals-nu": ([2] * 100, 100, False),
            "2nr-one-less-than-nu": ([2] * 99 + [3], 100, True)}


def _single_batch(u, rng):
    """one batch of (N, epb) = RUN_RULE whose distinct dofs are exactly ``u``"""
    N, epb = pm.RUN_RULE
    ent = np.concatenate([u, rng.choice(u, size=N * epb - u.size)]) if u.size < N * epb else u
    return np.ascontiguousarray(rng.permutation(ent).reshape(epb, N).astype(np.int32))


@pytest.mark.parametrize("case", sorted(RUN_RULE))
def test_run_rule(gpu, case):
    """a batch keeps a run table iff nr <= 128 and 2 nr < nu: both sides of both bounds"""
    _, L = gpu
    lengths, nr, table = RUN_RULE[case]
    dm = _single_batch(_runs_of(lengths), np.random.default_rng(len(case)))
    with _built(L, dm, pm.RUN_RULE[1]) as (p, _):
        assert p.nbatch == 1 and int(p.nr[0]) == nr and int(p.nu_count[0]) == sum(lengths) and bool(p.use_runs[0]) == table
        assert int(p.nu[0]) >> 16 == (nr if table else 0) and int(p.header[7]) == int(table)


def test_no_run_tables_when_the_build_is_told_so(gpu):
    lib, L = gpu
    old = lib.get_tuning(lib.TUNE_PLAN_RUNS)
    lib.set_tuning(lib.TUNE_PLAN_RUNS, 0)
    try:
        dm = _single_batch(_runs_of([4] * 128), np.random.default_rng(1))
        with _built(L, dm, pm.RUN_RULE[1], allow_runs=False) as (p, ws):
            got = _host(ws)
            lay = p.layout
            assert not (got[lay["nu"]:lay["nu"] + 4].view(np.int32) >> 16).any() and not got[lay["runs"]:lay["runs"] + lay["size"]["runs"]].any()
            assert int(got[:256].view(np.int64)[7]) == 0
        N, epb = 27, 19
        with _built(L, _edge_dofmap(N, epb, "structured"), epb, allow_runs=False) as (p, ws):
            h = _host(ws)[:256].view(np.int64)
            assert (int(h[7]), int(h[9]), int(h[11])) == (0, 128, 128) and int(h[8]) == 1
    finally:
        lib.set_tuning(lib.TUNE_PLAN_RUNS, old)


# ---- 5: the grid-stride loops of the two follow-up kernels ------------------------------------------------------------------------

def test_count_runs_takes_a_second_iteration(gpu):
    """300 000 batches of one entity: plan_count_runs_kernel (1024 x 256 threads) loops.  The workspace is 0.3 GB (a 1 kB run table per
    batch): the header and ``nu`` in full, the other regions in a strided sample of 1000 batches."""
    import torch

    _, L = gpu
    N, epb, nent = pm.GRID_STRIDE_COUNT
    dm = (np.arange(nent, dtype=np.int64)[:, None] * N + np.arange(N)).astype(np.int32)
    lay = pm.batch_layout(N, epb, nent)
    nbytes = int(L.fus_plan_bytes(N, epb, nent))
    assert nbytes == lay["bytes"] and lay["nbatch"] == nent > 1024 * 256
    nu, nr = pm.batch_counts(dm, epb)
    assert (nu == 4).all() and (nr == 1).all()
    dm_d = _dev(dm)
    with _workspace(L, nbytes) as ws:
        assert L.fus_plan_build(dm_d.data_ptr(), N, epb, nent, ws.data_ptr(), nbytes, None) == 0
        torch.cuda.synchronize()
        header = ws[:256].cpu().numpy()
        want = np.array([pm.PLAN_MAGIC, N, epb, nent, nent, N * epb, 0, nent, 0, 128, 0, 0], np.int64)
        assert header[:96].tobytes() == want.tobytes() and (header[96:] == FILL).all()
        got_nu = ws[lay["nu"]:lay["nu"] + 4 * nent].cpu().numpy().view(np.int32)
        assert got_nu.tobytes() == (nu | (nr << 16)).astype(np.int32).tobytes(), f"nu, first in batch {int(np.nonzero(got_nu != (nu | (nr << 16)))[0][0])}"
        sample = np.unique(np.concatenate([np.arange(0, nent, 301), [262143, 262144, nent - 1]]))
        assert sample.size == 1000
        p = pm.batch_plan(dm[sample], epb)  # epb = 1: the batches of the sample are batches of the plan
        idx = torch.from_numpy(sample).cuda()
        for name, row in (("udofs", p.udofs), ("runs", p.runs), ("slot", p.slot)):
            width = lay["size"][name] // nent
            got = ws[lay[name]:lay[name] + lay["size"][name]].view(nent, width)[idx].cpu().numpy()
            bad = np.nonzero((got != row.view(np.uint8).reshape(sample.size, width)).any(axis=1))[0]
            assert bad.size == 0, f"region '{name}' differs from the model, first in batch {int(sample[bad[0]])}"
        assert (ws[nbytes:] == FILL).all().item() and (ws[lay["order"]:lay["order"] + 4 * nent] == FILL).all().item()
        nb, wr = C.c_int64(-1), C.c_int64(-1)
        assert L.fus_plan_encoding(ws.data_ptr(), C.byref(nb), C.byref(wr), None, None) == 0 and (nb.value, wr.value) == (nent, nent)


def test_finish_takes_a_second_iteration(gpu):
    """4100 batches of P = 1 cells, one batch of scattered dofs (no table: the compact tables keep the full stride of 128):
    plan_finish_kernel (4096 x 256 threads) copies more than 2^20 words.  Everything compared in full."""
    _, L = gpu
    N, epb, nbatch = 8, pm.cells_per_batch(1), pm.GRID_STRIDE_FINISH_BATCHES
    assert int(L.fus_plan_entities_per_batch(N)) == epb
    dm = pm.dof_pattern("structured", N, nbatch * epb, N * epb).astype(np.int64)
    b = 2049
    dm[b * epb:(b + 1) * epb] = int(dm.max()) + 10 + 2 * np.arange(N * epb).reshape(epb, N)
    with _built(L, dm.astype(np.int32), epb) as (p, _):
        assert p.run_stride == 128 and p.nbatch * 2 * p.run_stride > 4096 * 256 and int(p.header[7]) == nbatch - 1
        assert p.mask[p.layout["runs_c"]:p.layout["runs_c"] + p.layout["size"]["runs_c"]].all()


# ---- 6: exclusive-dof marks -----------------------------------------------------------------------------------------------------

def _mark_cases():
    out = {}
    for N, epb in pm.DISPATCH_EDGES:
        for pattern in ("collide", "structured"):
            out[f"M{N * epb}-{pattern}"] = (lambda N=N, epb=epb, pattern=pattern: (_edge_dofmap(N, epb, pattern), epb, None, None))
    for P in (2, 4, 6):
        out[f"P{P}"] = (lambda P=P: (_box_dofmap(P)[0], pm.cells_per_batch(P), None, P))
    for N, epb in pm.ORDERED:
        out[f"ordered-{N}x{epb}"] = (lambda N=N, epb=epb: (_edge_dofmap(N, epb, "structured"), epb,
                                                            np.random.default_rng(N).permutation(pm.three_batches(epb)).astype(np.int32), None))
    return out


MARK_CASES = _mark_cases()


@pytest.mark.parametrize("case", sorted(MARK_CASES))
def test_exclusive_marks(gpu, case):
    """bit s of batch b iff dof s of the batch is inside the vector and nothing else -- no other batch, nothing the caller declared --
    touches it; ``use`` afterwards counts every (batch, dof).  A mark too many turns an atomic into a racing load + store, which a
    tolerance on the apply sees only sometimes: the words are compared exactly."""
    _, L = gpu
    dm, epb, order, P = MARK_CASES[case]()
    nent, N = dm.shape
    top = int(dm.max()) + 1
    rng = np.random.default_rng(len(case))
    with _built(L, dm, epb, order=order, P=P) as (p, ws):
        shared = np.bincount(np.concatenate(p.u))
        for what, ndofs, ext in (("alone", top, np.zeros(top, np.int32)), ("random", top, rng.integers(0, 2, size=top).astype(np.int32)),
                                 ("all-used", top, np.ones(top, np.int32)),
                                 ("short-vector", top - top // 3, rng.integers(0, 2, size=top - top // 3).astype(np.int32))):
            use, excl = pm.exclusive_marks(p, ndofs, ext)
            use_d = _dev(ext)
            assert L.fus_plan_mark_exclusive(ws.data_ptr(), N, epb, nent, use_d.data_ptr(), ndofs, None) == 0
            got_use = _host(use_d)
            assert got_use.shape == use.shape and got_use.tobytes() == use.tobytes(), f"{what}: use, first at dof {int(np.nonzero(got_use != use)[0][0])}"
            _assert_image(_host(ws), p, _batch_regions(p), f"{case}, {what}")
            marked = int(sum(bin(int(w)).count("1") for w in excl.reshape(-1)))
            if what == "alone":
                assert marked == int((shared == 1).sum()) and 0 < marked
                assert (shared > 1).any() and marked < int(p.nu_count.sum()), "the case has dofs that two batches share"
            if what == "all-used":
                assert marked == 0
            if what == "short-vector":
                assert int(np.concatenate(p.u).max()) >= ndofs


# ---- 7: no entities -------------------------------------------------------------------------------------------------------------

def test_zero_entities(gpu):
    _, L = gpu
    N, epb = 27, 19
    p = pm.batch_plan(np.zeros((0, N), np.int32), epb)
    nbytes = int(L.fus_plan_bytes(N, epb, 0))
    assert nbytes == p.layout["bytes"] == 256
    use = _dev(np.full(4, 7, np.int32))
    with _workspace(L, nbytes) as ws:
        assert L.fus_plan_build(None, N, epb, 0, ws.data_ptr(), nbytes, None) == 0
        assert L.fus_plan_mark_exclusive(ws.data_ptr(), N, epb, 0, use.data_ptr(), 4, None) == 0
        nb, wr = C.c_int64(-1), C.c_int64(-1)
        assert L.fus_plan_encoding(ws.data_ptr(), C.byref(nb), C.byref(wr), None, None) == 0 and (nb.value, wr.value) == (0, 0)
        assert (_host(ws) == FILL).all() and (_host(use) == 7).all()


# ---- 8 - 11: the transposed gather plan and its static companion ------------------------------------------------------------------

GATHER_NAMES = ("off_rows", "off_len", "off_base", "off_entries")
STATIC_NAMES = ("detJ_sorted", "ent16", "ent_base")


def _odd_dofmap():
    rng = np.random.default_rng(8)
    return (2 * rng.integers(0, 700, size=(300, 8)) + 1).astype(np.int32), 1500


def _hot_dofmap(entries):
    """dof 3 in ``entries`` entries, the rest spread over 40 dofs"""
    dm = np.random.default_rng(entries).integers(4, 44, size=(200, 3)).astype(np.int32)
    dm.reshape(-1)[:entries] = 3
    return dm, 50


def _rows_dofmap(nrows):
    """``nrows`` touched dofs, one to three entries each, in a shuffled order"""
    rng = np.random.default_rng(nrows)
    d = np.concatenate([np.arange(nrows), rng.integers(0, nrows, size=2 * ((nrows + 1) // 2) + nrows % 2)])
    return rng.permutation(d).reshape(-1, 2 if d.size % 2 == 0 else 1).astype(np.int32), nrows + 5


GATHER_CASES = {**{f"seed{s}": (lambda s=s: (lambda r: (r[4], r[3]))(pm.gather_random_dofmap(s))) for s in range(6)},
                "box-P2-dense": lambda: (lambda m: (m.dofmap, m.ndofs))(pkg("boxmesh").BoxMesh(2, (3, 2, 4))),
                "odd-dofs-sparse": _odd_dofmap,
                "len-255": lambda: _hot_dofmap(255),
                **{f"rows-{n}": (lambda n=n: _rows_dofmap(n)) for n in (1, 256, 257)}}


def _build_gather(L, dm, ndofs, ws, row_set=None, want=0):
    nent, N = dm.shape
    nbytes = ws.numel() - GUARD
    dm_d = _dev(dm)
    if row_set is None:
        return L.fus_mass_gather_plan_build(dm_d.data_ptr(), N, nent, ndofs, ws.data_ptr(), nbytes, None)
    return L.fus_mass_gather_plan_build_rows(dm_d.data_ptr(), N, nent, ndofs, _dev(row_set).data_ptr(), want, ws.data_ptr(), nbytes, None)


def _gather_bytes(L, g):
    nbytes = int(L.fus_mass_gather_plan_bytes(g.N, g.nent, g.ndofs))
    assert nbytes == g.layout["bytes"]
    return nbytes


@contextlib.contextmanager
def _gather_built(gpu, dm, ndofs, what):
    """Builds the full gather plan on the device and compares it with the model; yields (model, workspace), workspace None for a
    dofmap both sides refuse.  Nothing reads a plan on the device before it has been compared."""
    lib, L = gpu
    g = pm.gather_plan(dm, ndofs)
    with _workspace(L, _gather_bytes(L, g)) as ws:
        rc = _build_gather(L, dm, ndofs, ws)
        if g.bad:
            assert rc == lib.ERR_UNSUPPORTED_ENTITY
            yield g, None
            return
        assert rc == 0
        _assert_image(_host(ws), g, _regions(g.layout, GATHER_NAMES, 1), what)
        yield g, ws


@pytest.mark.parametrize("case", sorted(GATHER_CASES))
def test_gather_plan(gpu, case):
    """header, rows (when the plan carries them), len, base and the used entries: sorted by dof, ties ascending -- the order that makes
    the apply bitwise reproducible"""
    _, L = gpu
    dm, ndofs = GATHER_CASES[case]()
    with _gather_built(gpu, dm, ndofs, case) as (g, ws):
        if ws is None:
            return
        info = (C.c_int64 * 4)()
        assert L.fus_mass_gather_plan_info(ws.data_ptr(), info) == 0 and list(info) == [g.nrows, g.dense, g.max_len, g.layout["bytes"]]
        if case == "box-P2-dense":
            assert g.dense == 1 and g.nrows == ndofs and g.max_len == 8
        if case == "odd-dofs-sparse":
            assert g.dense == 0 and (g.rows % 2 == 1).all()
        if case.startswith("rows-"):
            n = int(case[5:])
            assert g.nrows == n and g.nblocks == -(-n // 256) and g.base.size == g.nblocks + 1
        if case == "len-255":
            assert g.max_len == 255


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(GATHER_CASES))
def test_static_companion(gpu, case, dt):
    """ent_base, ent16 and detJ_sorted (a bitwise copy) of the companion of every plan above, and the span word behind the bases"""
    _, L = gpu
    dm, ndofs = GATHER_CASES[case]()
    with _gather_built(gpu, dm, ndofs, case) as (g, ws):
        if ws is None:
            return
        dj = np.random.default_rng(17).uniform(0.5, 1.5, size=dm.shape).astype(dt)
        s = pm.static_companion(g, dj)
        sfx = "f64" if dt == np.float64 else "f32"
        sbytes = int(L.fus_mass_gather_static_bytes(g.N, g.nent, dj.dtype.itemsize))
        assert sbytes == s.layout["bytes"] and not s.too_wide
        with _workspace(L, sbytes) as sws:
            assert getattr(L, f"fus_mass_gather_static_build_{sfx}")(ws.data_ptr(), _dev(dj).data_ptr(), sws.data_ptr(), sbytes, None) == 0
            _assert_image(_host(sws), s, _regions(s.layout, STATIC_NAMES, 1), f"{case}: static companion, {sfx}")


def test_a_dof_with_256_entries_is_refused(gpu):
    lib, L = gpu
    dm, ndofs = _hot_dofmap(256)
    g = pm.gather_plan(dm, ndofs)
    assert g.bad and not pm.gather_plan(*_hot_dofmap(255)).bad
    with _workspace(L, _gather_bytes(L, g)) as ws:
        assert _build_gather(L, dm, ndofs, ws) == lib.ERR_UNSUPPORTED_ENTITY
        assert (_host(ws)[-GUARD:] == FILL).all()


@pytest.mark.parametrize("which", ["random-0", "random-1", "nothing", "everything"])
@pytest.mark.parametrize("case", ["seed0", "seed3", "odd-dofs-sparse"])
def test_gather_row_subsets(gpu, case, which):
    """only the dofs of the subset get a row, every row still holds ALL its entries; a subset that keeps nothing has no rows; one that
    keeps everything drops no sentinel row"""
    _, L = gpu
    dm, ndofs = GATHER_CASES[case]()
    marks = {"nothing": np.ones(ndofs, np.uint8), "everything": np.zeros(ndofs, np.uint8)}.get(which)
    if marks is None:
        marks = (np.random.default_rng(2).random(ndofs) < 0.4).astype(np.uint8)
    want = 1 if which == "random-1" else 0
    g = pm.gather_plan(dm, ndofs, marks, want)
    full = pm.gather_plan(dm, ndofs)
    assert not g.bad
    if which == "nothing":
        assert g.nrows == 0 and g.used == 0
    elif which == "everything":
        assert g.header.tobytes() == full.header.tobytes() and g.used == g.total and g.entries.tobytes() == full.entries.tobytes()
    else:
        assert 0 < g.nrows < full.nrows
    with _workspace(L, _gather_bytes(L, g)) as ws:
        assert _build_gather(L, dm, ndofs, ws, marks, want) == 0
        _assert_image(_host(ws), g, _regions(g.layout, GATHER_NAMES, 1), f"{case}, subset {which}")


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_static_companion_too_wide(gpu, dt):
    """block 0 holds the rows of entities 0 .. 127 and 69 000 .. 69 127: more than 65 535 apart.  The build is refused with
    FUS_ERR_UNSUPPORTED_ENTITY after the bases (and the span word behind them) were written; detJ_sorted and ent16 are untouched."""
    lib, L = gpu
    nent = 70_000
    e = np.arange(nent)
    dm = np.where(e < 1000, 2 * e, np.where(e >= 69_000, 2 * (e - 69_000) + 1, e + 1000)).astype(np.int32).reshape(nent, 1)
    assert (np.sort(dm.reshape(-1)) == e).all()
    g = pm.gather_plan(dm, nent)
    dj = np.random.default_rng(4).uniform(0.5, 1.5, size=dm.shape).astype(dt)
    s = pm.static_companion(g, dj)
    assert s.too_wide and s.span == 69_127 and g.dense == 1
    assert not s.mask[:s.layout["ent_base"]].any() and s.mask[s.layout["ent_base"]:s.layout["ent_base"] + 4 * (g.nblocks + 1)].all()
    sfx = "f64" if dt == np.float64 else "f32"
    with _workspace(L, _gather_bytes(L, g)) as ws:
        assert _build_gather(L, dm, nent, ws) == 0
        _assert_image(_host(ws), g, _regions(g.layout, GATHER_NAMES, 1), "wide plan")
        sbytes = int(L.fus_mass_gather_static_bytes(1, nent, dj.dtype.itemsize))
        assert sbytes == s.layout["bytes"]
        with _workspace(L, sbytes) as sws:
            rc = getattr(L, f"fus_mass_gather_static_build_{sfx}")(ws.data_ptr(), _dev(dj).data_ptr(), sws.data_ptr(), sbytes, None)
            assert rc == lib.ERR_UNSUPPORTED_ENTITY
            _assert_image(_host(sws), s, _regions(s.layout, STATIC_NAMES, 1), f"too wide, {sfx}")
