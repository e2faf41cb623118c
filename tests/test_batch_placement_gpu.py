"""The general-G planned apply with its batches placed in groups on the XCDs (csrc/stiffness.hpp: ``group_block``; knob
``TUNE_PLAN_XCD_GROUP``; the map itself: tests/test_batch_placement.py).

The kernels can only go wrong where the batch count meets a boundary of the super-groups of 8 g batches (a batch run twice or never), so
the meshes are the smallest there: P = 4 (10 cells per batch), g = 2 with 1, 7, 9, 15, 16, 17 batches and g = 4 with 31, 32, 33; one case
each of P = 2 (28 cells per batch), P = 7 (4 per batch), the fp32 twin kernel, the slot kernel (``TUNE_PLAN_ROWS`` = 0), an ordered plan and
a group size far above the batch count.  Every case: y against ``oracle_c.stiffness_apply`` with the ``_check`` rule of
tests/test_plan_rows_gpu.py (fp64: rel l2 < 1e-12, rel max < 1e-11; fp32: 1e-5, 1e-4), and y against the natural order's y under the
same rule (the placement changes only the order in which the batches' sums reach y)."""
import numpy as np
import pytest

from conftest import TOL, build_problem, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -1  # include/fus_gpu.h: FUS_ERR_INVALID_ARGUMENT

# (id, P, cells, dtype, g, batches, rows knob, shuffled cells)
CASES = [(f"g2_{nb}_batches", 4, cells, np.float64, 2, nb, 1, False)
         for nb, cells in ((1, (2, 2, 2)), (7, (2, 5, 7)), (9, (3, 5, 6)), (15, (5, 5, 6)), (16, (4, 5, 8)), (17, (4, 6, 7)))]
CASES += [(f"g4_{nb}_batches", 4, cells, np.float64, 4, nb, 1, False) for nb, cells in ((31, (2, 5, 31)), (32, (4, 8, 10)), (33, (5, 6, 11)))]
CASES += [("P2", 2, (6, 7, 11), np.float64, 2, 17, 1, False),
          ("P7", 7, (2, 2, 17), np.float64, 2, 17, 1, False),
          ("fp32_twin", 4, (4, 6, 7), np.float32, 2, 17, 1, False),
          ("slot_kernel", 4, (4, 6, 7), np.float64, 2, 17, 0, False),
          ("ordered_plan", 4, (4, 6, 7), np.float64, 2, 17, 1, True),
          ("g256_on_17_batches", 4, (4, 6, 7), np.float64, 256, 17, 1, False)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    torch.cuda.set_device(0)
    return pkg("device"), pkg("operators")


@pytest.fixture(autouse=True)
def _restore(gpu):
    _, ops = gpu
    lib = pkg("_lib")
    old = {k: lib.get_tuning(k) for k in (lib.TUNE_PLAN_XCD_GROUP, lib.TUNE_PLAN_ROWS, lib.TUNE_XCD_REMAP)}
    ops._PLANS.clear()
    ops.use_plan(True)
    yield
    for k, v in old.items():
        lib.set_tuning(k, v)
    ops._PLANS.clear()


_problems = {}


def _problem(P, cells, dtype, shuffled, oracle_c):
    """one problem and its oracle result per shape, built once and left unchanged"""
    key = (P, cells, np.dtype(dtype).name, shuffled)
    if key not in _problems:
        pb = build_problem(P, cells, dtype=dtype, perturb=0.16, seed=11)
        mesh = pb["mesh"]
        dm, G, cc = mesh.dofmap, pb["G"], pb["cc"]
        if shuffled:
            perm = np.random.default_rng(3).permutation(mesh.ncells)
            dm, G, cc = (np.ascontiguousarray(a[perm]) for a in (dm, G, cc))
        y_ref = np.zeros(mesh.ndofs, dtype=dtype)
        oracle_c.stiffness_apply(P, pb["D"], pb["x"], cc, y_ref, G, dm)
        _problems[key] = (pb, dm, G, cc, y_ref)
    return _problems[key]


def _check(got, ref, dtype, what):
    tol = TOL[np.dtype(dtype)]
    e2, em = rel_l2(got, ref), rel_max(got, ref)
    assert e2 < tol["l2"] and em < tol["mx"], f"{what}: rel l2 {e2:.3e} (tol {tol['l2']}), rel max {em:.3e}"


def _stiffness(gpu, pb, dtype, dm, G, cc):
    dev, ops = gpu
    y = dev.to_device(np.zeros(pb["mesh"].ndofs, dtype=dtype))
    ops.stiffness_operator(pb["P"], pb["D"].flatten(), dtype)(dev.to_device(pb["x"]), dev.to_device(cc), y, dev.to_device(G), dev.to_device(dm))
    return y.copy_to_host()


@pytest.mark.parametrize("name,P,cells,dtype,g,nbatch,rows,shuffled", CASES, ids=[c[0] for c in CASES])
def test_grouped_placement_gives_the_natural_orders_result(gpu, oracle_c, name, P, cells, dtype, g, nbatch, rows, shuffled):
    _, ops = gpu
    lib = pkg("_lib")
    pb, dm, G, cc, y_ref = _problem(P, cells, dtype, shuffled, oracle_c)
    epb = max(256 // (P + 1) ** 2, 1)
    assert -(-pb["mesh"].ncells // epb) == nbatch, "the mesh must give the batch count the case is about"
    lib.set_tuning(lib.TUNE_PLAN_ROWS, rows)
    ys = {}
    for knob in (0, g):
        lib.set_tuning(lib.TUNE_PLAN_XCD_GROUP, knob)
        assert lib.get_tuning(lib.TUNE_PLAN_XCD_GROUP) == knob
        ys[knob] = _stiffness(gpu, pb, dtype, dm, G, cc)
        _check(ys[knob], y_ref, dtype, f"{name}: group knob {knob} against the oracle")
    if shuffled:
        assert ops._PLANS.last_order is not None, "the random cell order must have triggered the locality plan"
    _check(ys[g], ys[0], dtype, f"{name}: g = {g} against the natural order")


def test_knob_round_trip_and_refusals():
    lib = pkg("_lib")
    clib = lib.load()
    key = lib.TUNE_PLAN_XCD_GROUP
    assert key == 8
    assert lib.get_tuning(key) == -1, "the default is auto"
    for v in (0, 2, 4, 8, 16, 32, 64, 128, 256, -1):
        lib.set_tuning(key, v)
        assert lib.get_tuning(key) == v
    lib.set_tuning(key, 16)
    for bad in (1, 3, 6, 12, 48, 255, 257, 512, 1024, -2, -16):
        assert clib.fus_set_tuning(key, bad) == INVALID_ARGUMENT, bad
        assert lib.get_tuning(key) == 16, "a refused value leaves the knob as it was"
    # the old mode keeps its 0 / 1 meaning beside it
    lib.set_tuning(lib.TUNE_XCD_REMAP, 1)
    assert lib.get_tuning(lib.TUNE_XCD_REMAP) == 1 and lib.get_tuning(key) == 16
    assert clib.fus_abi_version() == 3


def test_whole_chunks_mode_wins_over_the_groups(gpu, oracle_c):
    """``TUNE_XCD_REMAP`` = 1 with a group size set: the launch takes the contiguous eighths (17 batches: 3, 2, 2, ... per XCD label)"""
    lib = pkg("_lib")
    pb, dm, G, cc, y_ref = _problem(4, (4, 6, 7), np.float64, False, oracle_c)
    lib.set_tuning(lib.TUNE_PLAN_XCD_GROUP, 2)
    lib.set_tuning(lib.TUNE_XCD_REMAP, 1)
    _check(_stiffness(gpu, pb, np.float64, dm, G, cc), y_ref, np.float64, "whole chunks with a group size set")
