"""The index model of the two plans (tests/plan_model.py) on the CPU: that it is consistent with what a plan MEANS (a slot names the
entry's dof, a run table expands to the dof list, the marks are the dofs of exactly one batch, the gather plan sums what the dofmap
sums); that the builder kernels the library compiles are exactly the ones the model speaks of (from the kernel names of a device-only
compile: no GPU); and that the cases of tests/test_plan_builders_gpu.py reach every build of the sort kernel."""
import collections
import os
import re
import shutil
import sys

import numpy as np
import pytest

import plan_model as pm
from conftest import ROOT, pkg

_BUILDER = re.compile(r"fus::((?:plan_build|plan_count_runs|plan_finish|plan_count_uses|plan_mark_exclusive|gather_iota|gather_flag|gather_rows|gather_len"
                      r"|gather_subset_keys|gather_static_base|gather_static_fill)_kernel)(?:<(\w+)>)?\(")
BUILDERS = ([("plan_build_kernel", str(m)) for m in pm.SORT_SIZES]
            + [(k, None) for k in ("plan_count_runs_kernel", "plan_finish_kernel", "plan_count_uses_kernel", "plan_mark_exclusive_kernel", "gather_iota_kernel",
                                   "gather_flag_kernel", "gather_rows_kernel", "gather_len_kernel", "gather_subset_keys_kernel", "gather_static_base_kernel")]
            + [("gather_static_fill_kernel", t) for t in ("float", "double")])


def _box_dofmap():
    return pkg("boxmesh").BoxMesh(4, (3, 2, 7)).dofmap


def _collide_dofmap():
    return pm.dof_pattern("collide", 27, pm.three_batches(19), 27 * 19, seed=3)


DOFMAPS = {"box-P4": (_box_dofmap, pm.cells_per_batch(4)), "collide": (_collide_dofmap, 19)}


@pytest.fixture(scope="module", params=sorted(DOFMAPS))
def plan(request):
    make, epb = DOFMAPS[request.param]
    dofmap = make()
    return dofmap, pm.batch_plan(dofmap, epb)


def test_a_slot_names_the_dof_of_its_entry(plan):
    dofmap, p = plan
    assert p.nbatch >= 3 and p.nent % p.epb != 0, "several batches, the last one ragged"
    for b in range(p.nbatch):
        ent = dofmap[b * p.epb:(b + 1) * p.epb].reshape(-1)
        assert (p.udofs[b][p.slot[b, :ent.size]] == ent).all()
        nu = int(p.nu[b]) & 0xFFFF
        assert nu == np.unique(ent).size and (np.diff(p.udofs[b, :nu]) > 0).all() and (p.udofs[b, nu:] == p.udofs[b, 0]).all()


def test_the_run_table_expands_to_the_dof_list(plan):
    _, p = plan
    assert p.use_runs.any()
    for b in range(p.nbatch):
        nu, nr = int(p.nu[b]) & 0xFFFF, int(p.nu[b]) >> 16
        assert nr == (p.nr[b] if p.use_runs[b] else 0)
        if nr == 0:
            assert not p.runs[b].any()
            continue
        first, at = p.runs[b, 0:2 * nr:2], p.runs[b, 1:2 * nr:2]
        ends = np.append(at[1:], nu)
        assert (np.concatenate([d + np.arange(e - s) for d, s, e in zip(first, at, ends)]) == p.udofs[b, :nu]).all()
        assert not p.runs[b, 2 * nr:].any()
        if p.row_len:
            assert (p.runs_c[b] == p.runs[b, :2 * p.run_stride]).all() and 2 * p.run_stride >= 2 * nr


def test_consecutive_rows_have_consecutive_slots():
    dofmap = _box_dofmap()
    p = pm.batch_plan(dofmap, pm.cells_per_batch(4))
    n = p.row_len
    assert n == 5 and p.rows_consecutive == 1 and p.header[10] == 0 and p.header[11] <= p.run_stride < 2 * p.header[11]
    for b in range(p.nbatch):
        valid = dofmap[b * p.epb:(b + 1) * p.epb].size
        assert (p.slot[b, :valid].reshape(-1, n) == p.rowbase[b, :valid // n, None] + np.arange(n)).all()
    q = pm.batch_plan(_collide_dofmap(), 19)
    assert q.row_len == 3 and q.rows_consecutive == 0 and q.header[10] == 1


def test_the_marks_are_the_dofs_of_exactly_one_batch(plan):
    dofmap, p = plan
    ndofs = int(dofmap.max()) + 1 - 7  # the largest dofs lie outside the vector: neither counted nor marked
    ext = np.random.default_rng(5).integers(0, 2, size=ndofs)
    use, excl = pm.exclusive_marks(p, ndofs, ext)
    sets = [set(int(d) for d in dofmap[b * p.epb:(b + 1) * p.epb].reshape(-1)) for b in range(p.nbatch)]
    count = collections.Counter(d for s in sets for d in s)
    assert all(use[d] == ext[d] + count.get(d, 0) for d in range(ndofs))
    marked = 0
    for b, s in enumerate(sets):
        for k, d in enumerate(sorted(s)):
            bit = (int(excl[b, k // 32]) >> (k % 32)) & 1
            assert bit == int(d < ndofs and ext[d] == 0 and count[d] == 1), (b, k, d)
            marked += bit
        assert all(((int(excl[b, k // 32]) >> (k % 32)) & 1) == 0 for k in range(len(s), 32 * excl.shape[1]))
    assert marked > 0
    assert not pm.exclusive_marks(p, ndofs, np.ones(ndofs, np.int32))[1].any()


@pytest.mark.parametrize("subset", [None, 0, 1])
def test_the_gather_plan_sums_what_the_dofmap_sums(plan, subset):
    dofmap, _ = plan
    ndofs = int(dofmap.max()) + 3
    rng = np.random.default_rng(9)
    marks = (rng.random(ndofs) < 0.4).astype(np.uint8)
    g = pm.gather_plan(dofmap, ndofs) if subset is None else pm.gather_plan(dofmap, ndofs, marks, subset)
    assert not g.bad and g.base[-1] == g.used == int(g.len.sum()) and (np.diff(g.rows) > 0).all()
    v = rng.standard_normal(dofmap.size)
    ref = np.zeros(ndofs)
    np.add.at(ref, dofmap.reshape(-1), v)
    if subset is not None:
        ref[marks != subset] = 0.0
    got = np.zeros(ndofs)
    np.add.at(got, np.repeat(g.rows, g.len), v[g.entries])
    assert np.array_equal(got, ref), "the same terms in the same (ascending entry) order: bitwise"
    assert (dofmap.reshape(-1)[g.entries] == np.repeat(g.rows, g.len)).all()
    start = np.concatenate([[0], np.cumsum(g.len.astype(np.int64))])
    assert all((np.diff(g.entries[a:b]) > 0).all() for a, b in zip(start[:-1], start[1:])), "ties ascending"
    assert (g.base[:-1] == start[:-1][::256]).all()
    # the companion: the entity of every entry from its block's base and a 16-bit offset
    dj = rng.standard_normal(dofmap.shape)
    s = pm.static_companion(g, dj)
    assert not s.too_wide
    block = np.repeat(np.arange(g.nblocks), np.diff(g.base))
    assert (s.ent_base[block] + s.ent16 == g.entries // g.N).all() and s.detJ_sorted.tobytes() == dj.reshape(-1)[g.entries].tobytes()


def test_what_the_gather_plan_refuses():
    dm = np.zeros((256, 1), np.int32)
    assert pm.gather_plan(dm, 4).bad and pm.gather_plan(dm[:255], 4).max_len == 255
    assert pm.gather_plan(np.array([[0, 4]], np.int32), 4).bad and pm.gather_plan(np.array([[0, -1]], np.int32), 4).bad
    # a hot dof outside the subset is nobody's row: not refused
    assert not pm.gather_plan(dm, 4, np.ones(4, np.uint8), 0).bad and pm.gather_plan(dm, 4, np.ones(4, np.uint8), 0).nrows == 0


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_the_builder_kernels_are_what_the_library_compiles():
    """Both ways: a builder instantiation added to the library without a word in the model fails here, and so does a kernel the model
    names that no compile produces."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    compiled = [(m.group(1), m.group(2)) for m in (_BUILDER.search(name) for name in ru.parse(ru.cached_remarks())) if m]
    assert len(compiled) == len(set(compiled)), "a builder kernel occurs twice"
    missing, unknown = sorted(set(compiled) - set(BUILDERS), key=repr), sorted(set(BUILDERS) - set(compiled), key=repr)
    assert not missing, f"compiled builder kernels the model does not name: {missing}"
    assert not unknown, f"builder kernels of the model that the library does not compile: {unknown}"
    assert len(compiled) == 17


def test_the_cases_reach_every_sort_size():
    shapes = pm.case_shapes()
    sizes = collections.Counter(pm.sort_size(N * epb) for _, N, epb in shapes)
    assert set(sizes) == set(pm.SORT_SIZES) and all(sizes[m] >= 2 for m in pm.SORT_SIZES), sizes
    assert [N * epb for N, epb in pm.DISPATCH_EDGES] == [256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096]
    assert [pm.sort_size(m) for m in (1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)] == [256, 256, 512, 512, 1024, 1024, 2048, 2048, 4096, 4096]
    assert pm.sort_size(241 * 17) is None and 241 * 17 == 4097 and pm.sort_size(0) is None
    assert {pm.plan_row_len(N) > 0 for N, _ in pm.DISPATCH_EDGES} == {True, False}, "cell and other plans mixed"
    assert [pm.plan_row_len(N) for N in (1, 2, 8, 9, 27, 64, 1331)] == [1, 0, 2, 0, 3, 4, 11]
    assert [pm.cells_per_batch(P) for P in pm.CELL_DEGREES] == [64, 28, 16, 10, 7, 5, 4, 3, 2, 2]
    # the two grid-stride loops: plan_count_runs_kernel runs 1024 x 256 threads, plan_finish_kernel 4096 x 256
    N, epb, nent = pm.GRID_STRIDE_COUNT
    assert -(-nent // epb) > 1024 * 256
    assert pm.GRID_STRIDE_FINISH_BATCHES * 2 * pm.PLAN_MAX_RUNS > 4096 * 256


def test_the_layout_of_a_plan_without_cells_has_no_row_regions():
    lay = pm.batch_layout(25, 41, 100)
    assert "rowbase" not in lay and "runs_c" not in lay and lay["bytes"] == lay["excl"] + pm.align256(lay["size"]["excl"])
    cell = pm.batch_layout(27, 19, 100)
    assert cell["order"] < cell["rowbase"] < cell["runs_c"] < cell["excl"] and all(cell[k] % 256 == 0 for k in cell["size"])
    assert pm.batch_layout(1, 3, 7)["row_len"] == 1
    p = pm.batch_plan(pm.dof_pattern("structured", 25, 100, 25 * 41), 41)
    assert p.header[8] == 0 and p.header[9] == 128 and p.header[10] == 0 and p.header[11] == 0
    assert pm.batch_plan(np.zeros((0, 8), np.int32), 4).mask.sum() == 0
