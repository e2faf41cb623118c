"""The general-G planned apply walking its batches downwards or in alternating directions (csrc/stiffness.hpp: ``mirror_block``, the flag
bit of ``place_batch``; the parity: csrc/plan_registry.hpp ``flip_sweep``; knob ``TUNE_PLAN_SWEEP``; the map itself and the parity on the
host: tests/test_sweep_placement.py).

The mirrored launch can only go wrong where the mirror meets the placement and the ragged end of the plan, so the meshes are the smallest
there: P = 4 with 14^3 = 2744 cells (275 batches: one whole super-group of 256 at g = 32, a tail of 19, a last batch with 4 of 10 cells,
which workgroup 0 now runs) and 7 x 6 x 5 = 210 cells (every g above the grid: natural order); P = 8 (3 cells per batch) and P = 2 (28) at
a few thousand cells with a ragged last batch; the fp32 kernel at P = 3; a randomly renumbered dofmap (``stiffness_plan_kernel`` instead of
the rows kernel) and a plan with a cell order.  Every case, against ``oracle_c.stiffness_apply`` with the ``_check`` rule of
tests/test_plan_rows_gpu.py and tests/test_batch_placement_gpu.py (fp64: rel l2 < 1e-12, rel max < 1e-11; fp32: 1e-5, 1e-4):
  * knob 0 (upwards) and knob 2 (downwards) give K x;
  * knob 1 applied three times into one y gives 3 K x (up, down, up on one plan);
  * knob -1: these launches are below half of the 256 MiB of the byte rule (benchlib.roofline.stiffness_bytes_per_cell x cells; the rule in
    C++: tests/host/plan_sweep_check.cpp), so auto walks upwards: the knob reads -1, the rule says no, and the result is K x;
  * two applies captured in one ``torch.cuda.graph`` under knob 1 and replayed three times give 6 K x.
Nothing here is timed."""
import numpy as np
import pytest

from conftest import TOL, build_problem, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -1  # include/fus_gpu.h: FUS_ERR_INVALID_ARGUMENT

# (id, P, cells, dtype, batches, kind): kind "box" the mesh's own numbering, "renumbered" a random dof numbering, "shuffled" a random cell order
CASES = [("P4_275_batches", 4, (14, 14, 14), np.float64, 275, "box"),
         ("P4_21_batches", 4, (7, 6, 5), np.float64, 21, "box"),
         ("P8", 8, (13, 11, 14), np.float64, 668, "box"),
         ("P2", 2, (13, 13, 13), np.float64, 79, "box"),
         ("fp32_P3", 3, (11, 11, 11), np.float32, 84, "box"),
         ("renumbered_slot_kernel", 4, (7, 6, 5), np.float64, 21, "renumbered"),
         ("ordered_plan", 4, (7, 6, 5), np.float64, 21, "shuffled")]


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
    old = {k: lib.get_tuning(k) for k in (lib.TUNE_PLAN_SWEEP, lib.TUNE_PLAN_XCD_GROUP, lib.TUNE_PLAN_ROWS, lib.TUNE_XCD_REMAP)}
    ops._PLANS.clear()
    ops.use_plan(True)
    yield
    for k, v in old.items():
        lib.set_tuning(k, v)
    ops._PLANS.clear()


_problems = {}


def _problem(P, cells, dtype, kind, oracle_c):
    """one problem and its oracle result per case, built once and left unchanged: (pb, dofmap, G, cc, x, K x)"""
    key = (P, cells, np.dtype(dtype).name, kind)
    if key not in _problems:
        pb = build_problem(P, cells, dtype=dtype, perturb=0.16, seed=11)
        mesh = pb["mesh"]
        dm, G, cc, x = mesh.dofmap, pb["G"], pb["cc"], pb["x"]
        if kind == "shuffled":
            perm = np.random.default_rng(3).permutation(mesh.ncells)
            dm, G, cc = (np.ascontiguousarray(a[perm]) for a in (dm, G, cc))
        elif kind == "renumbered":  # new = perm[old]
            perm = np.random.default_rng(3).permutation(mesh.ndofs).astype(dm.dtype)
            x = np.empty_like(pb["x"])
            x[perm] = pb["x"]
            dm = np.ascontiguousarray(perm[dm])
        y_ref = np.zeros(mesh.ndofs, dtype=dtype)
        oracle_c.stiffness_apply(P, pb["D"], x, cc, y_ref, G, dm)
        _problems[key] = (pb, dm, G, cc, x, y_ref)
    return _problems[key]


def _check(got, ref, dtype, what):
    tol = TOL[np.dtype(dtype)]
    e2, em = rel_l2(got, ref), rel_max(got, ref)
    assert e2 < tol["l2"] and em < tol["mx"], f"{what}: rel l2 {e2:.3e} (tol {tol['l2']}), rel max {em:.3e}"


class _Apply:
    """One operator on one set of device arrays: every call is a launch on the SAME plan (the plan cache keys on the dofmap's address)."""

    def __init__(self, gpu, pb, dtype, dm, G, cc, x):
        dev, ops = gpu
        self.op = ops.stiffness_operator(pb["P"], pb["D"].flatten(), dtype)
        self.x, self.cc, self.G, self.dm = dev.to_device(x), dev.to_device(cc), dev.to_device(G), dev.to_device(dm)
        self.y = dev.to_device(np.zeros(pb["mesh"].ndofs, dtype=dtype))

    def __call__(self, times=1):
        self.y.zero_()
        for _ in range(times):
            self.op(self.x, self.cc, self.y, self.G, self.dm)
        return self.y.copy_to_host()


@pytest.mark.parametrize("name,P,cells,dtype,nbatch,kind", CASES, ids=[c[0] for c in CASES])
def test_every_direction_gives_the_oracles_result(gpu, oracle_c, name, P, cells, dtype, nbatch, kind):
    import torch

    from benchlib.roofline import stiffness_bytes_per_cell

    _, ops = gpu
    lib = pkg("_lib")
    pb, dm, G, cc, x, y_ref = _problem(P, cells, dtype, kind, oracle_c)
    ncells = pb["mesh"].ncells
    epb = max(256 // (P + 1) ** 2, 1)
    assert -(-ncells // epb) == nbatch, "the mesh must give the batch count the case is about"
    if kind == "box" and nbatch > 21:
        assert ncells % epb != 0, "... and a ragged last batch"
    apply = _Apply(gpu, pb, dtype, dm, G, cc, x)

    # auto: the knob's default, and a launch below the cache walks upwards
    assert lib.get_tuning(lib.TUNE_PLAN_SWEEP) == -1, "the default is auto"
    assert stiffness_bytes_per_cell(P, np.dtype(dtype).itemsize) * ncells < (256 << 20) // 2, "the byte rule says no: auto = upwards"
    _check(apply(), y_ref, dtype, f"{name}: auto")
    if kind == "shuffled":
        assert ops._PLANS.last_order is not None, "the random cell order must have triggered the locality plan"
    if kind == "renumbered":
        ws = [v for k, v in ops._PLANS._plans.items() if k[-1] != "strips"][-1][0]
        assert int(ws[:256].cpu().numpy().view(np.int64)[8]) == 0, "a random numbering has no consecutive rows: the slot kernel runs"

    ys = {}
    for knob in (0, 2):
        lib.set_tuning(lib.TUNE_PLAN_SWEEP, knob)
        assert lib.get_tuning(lib.TUNE_PLAN_SWEEP) == knob
        ys[knob] = apply()
        _check(ys[knob], y_ref, dtype, f"{name}: sweep knob {knob} against the oracle")
    _check(ys[2], ys[0], dtype, f"{name}: downwards against upwards")

    lib.set_tuning(lib.TUNE_PLAN_SWEEP, 1)
    _check(apply(3), 3 * y_ref.astype(np.float64), dtype, f"{name}: three alternating applies")

    # two applies in one captured graph (the directions are fixed at capture: one up, one down), replayed three times
    apply()  # every kernel once outside the capture
    torch.cuda.synchronize()
    apply.y.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        apply.op(apply.x, apply.cc, apply.y, apply.G, apply.dm)
        apply.op(apply.x, apply.cc, apply.y, apply.G, apply.dm)
    apply.y.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    _check(apply.y.copy_to_host(), 6 * y_ref.astype(np.float64), dtype, f"{name}: two captured applies replayed three times")


def test_knob_round_trip_and_refusals():
    lib = pkg("_lib")
    clib = lib.load()
    key = lib.TUNE_PLAN_SWEEP
    assert key == 9
    assert lib.get_tuning(key) == -1, "the default is auto"
    for v in (0, 1, 2, -1):
        lib.set_tuning(key, v)
        assert lib.get_tuning(key) == v
    lib.set_tuning(key, 1)
    for bad in (3, 4, -2, 16, 1 << 16, -(1 << 16)):
        assert clib.fus_set_tuning(key, bad) == INVALID_ARGUMENT, bad
        assert lib.get_tuning(key) == 1, "a refused value leaves the knob as it was"
    # the placement knobs keep their values beside it
    assert lib.get_tuning(lib.TUNE_PLAN_XCD_GROUP) == -1 and lib.get_tuning(lib.TUNE_XCD_REMAP) == 0
    assert clib.fus_abi_version() == 3


def test_downwards_with_every_placement(gpu, oracle_c):
    """The mirror comes after the placement: downwards with the natural order, with groups of 2 and 32 (whole super-groups and a tail) and
    with the contiguous eighths of ``TUNE_XCD_REMAP`` = 1 (275 batches: 35, 35, 35, 34, ... per XCD label)."""
    lib = pkg("_lib")
    pb, dm, G, cc, x, y_ref = _problem(4, (14, 14, 14), np.float64, "box", oracle_c)
    apply = _Apply(gpu, pb, np.float64, dm, G, cc, x)
    lib.set_tuning(lib.TUNE_PLAN_SWEEP, 2)
    for group, chunks in ((0, 0), (2, 0), (32, 0), (32, 1)):
        lib.set_tuning(lib.TUNE_PLAN_XCD_GROUP, group)
        lib.set_tuning(lib.TUNE_XCD_REMAP, chunks)
        _check(apply(), y_ref, np.float64, f"downwards, group {group}, whole chunks {chunks}")
