"""Every shipped build of the streaming vector kernels (tests/stream_builds.py: 338 instantiations of ten kernels) against an fp64
statement of the same operation.

(a) One case per build at two sizes.  The small size is that of the kernel's own test (1027, or 1003 / 997 for bioheat) with its tail,
ghost block and guard elements, in every kind and output set that test runs.  The sweep size is ``stream_builds.sweep_size``: the grid
is at its cap and 777 or 778 threads take a SECOND iteration of the grid-stride loop, which no other kernel test reaches; there each
build runs once, the kinds, output sets and optional operands rotating over the builds of a kernel.  The gather sweeps rows
(``stream_builds.gather_rows``), the sponge a list of 2048 x 256 + 778 ascending indices into a vector three times as long.

(b) Reference and bounds: each kernel's existing fp64 numpy statement and bound, through the helper its own test calls
(``test_bioheat_gpu._stage_case``, ``test_relaxation_gpu._relax_stage_case``, ``test_field_monitor_gpu._kernel_case``,
``test_operators_gpu._rk4_table_case``, ``test_sponge_gpu._sponge_case``); the gather against ``np.add.at`` in fp64 at tol x max_len
(1e-13 / 2e-5), static bitwise equal to default; ``ew_kernel`` / ``muladd_kernel`` per element against fp64 numpy on the once-rounded
inputs (an fp64 kernel: against numpy's longdouble, 64 bits of mantissa on x86-64, since an fp64 reference would carry the very error
it is to measure -- the first run had the fp64 axpy and muladd AT their bound against fp64 numpy): copy and fill bitwise, scale / square
/ divide within eps |ref| (one rounding), axpy and muladd within eps (|alpha a| + |y|) (the FMA and the two-rounding form).  The divide
bound rests on clang's default of correctly rounded fp32 division for HIP (csrc/Makefile passes no flag that lifts it); measured: the
largest fp32 quotient error is 0.50 of the bound, half an ulp.  And for every NT != 0 build all outputs are BITWISE those of the NT = 0
build on the same inputs.

(c) The piece seam: one fp32 case per launcher that splits into launches of 2^27 dofs (the monitor, bioheat, relax), inputs drawn on
the device from seeded generators, the reference formed on the device in torch fp64 in chunks with the formulas and bounds of (b); only
the largest ratio of error to bound and the bitwise flags come back.  These skip only below 24 GB of free device memory.

(d) NOT asserted: which instantiation a launch chose -- the library offers no way to read that back.  Steering is by construction:
alignment, mode and flags go through csrc/stream_shape.hpp, which tests/host/stream_shape_check.cpp checks, and
tests/test_stream_builds.py ties ``steer`` to the compiled names through a restatement of those rules.

Every case prints its largest error as a ratio to its bound (profiles/stream_builds_errors.log is one run's output: ew / muladd up to
0.50, RK4 stages 0.21, bioheat 0.32, relax 0.17, monitor 0.29, gather 1.1e-4, sponge 7e-4; the seams 0.25, 0.83 (the dose against the
reference's) and 0.07).  Nothing is timed."""

import contextlib
import ctypes
import math

import numpy as np
import pytest

import stream_builds as sb
from conftest import pkg

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
GUARD, SENTINEL = 8, -7.25
SMALL = 1027


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    torch.cuda.set_device(0)
    return pkg("operators"), pkg("_lib")


@contextlib.contextmanager
def _tuned(vector_stream, mass_variant=None):
    """The tuning switches of a case, restored afterwards -- and asserted restored."""
    lib = pkg("_lib")
    knobs = [(lib.TUNE_VECTOR_STREAM, vector_stream)] + ([(lib.TUNE_MASS_VARIANT, mass_variant)] if mass_variant is not None else [])
    old = [lib.get_tuning(k) for k, _ in knobs]
    try:
        for k, v in knobs:
            lib.set_tuning(k, v)
        yield
    finally:
        for (k, _), v in zip(knobs, old):
            lib.set_tuning(k, v)
    assert [lib.get_tuning(k) for k, _ in knobs] == old


@pytest.fixture(autouse=True)
def _defaults_hold(gpu):
    _, lib = gpu
    before = (lib.get_tuning(lib.TUNE_VECTOR_STREAM), lib.get_tuning(lib.TUNE_MASS_VARIANT))
    yield
    assert (lib.get_tuning(lib.TUNE_VECTOR_STREAM), lib.get_tuning(lib.TUNE_MASS_VARIANT)) == before


def _builds(kernel, dtype, **flags):
    out = [b for b in sb.MATRIX if b.kernel == kernel and b.dtype == dtype and all(dict(b.flags)[k] == v for k, v in flags.items())]
    assert out
    return out


def _by_width(builds):
    """{W: [the NT = 0 build, then the others]} -- the cached build runs first: the others are compared with it bit for bit."""
    out = {}
    for b in sorted(builds, key=lambda b: (b.W, b.NT)):
        out.setdefault(b.W, []).append(b)
    assert all(bs[0].NT == 0 for bs in out.values())
    return out


def _index(b):
    """The position of ``b`` among the builds of its kernel: what the rotations of kinds and output sets count."""
    return [c for c in sb.MATRIX if c.kernel == b.kernel].index(b)


def _log(b, n, what, ratio):
    print(f"stream_builds {sb.case_id(b)} n {n} {what}: max err / bound {ratio:.3g}")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_same(ref, got, b, n, what=""):
    """Every output of an NT != 0 build is bitwise that of the NT = 0 build (same arithmetic, another access flavour)."""
    if isinstance(ref, dict):
        assert ref.keys() == got.keys()
        for k in ref:
            _assert_same(ref[k], got[k], b, n, f"{what} {k}")
    elif isinstance(ref, (list, tuple)):
        assert len(ref) == len(got)
        for i, (r, g) in enumerate(zip(ref, got)):
            _assert_same(r, g, b, n, f"{what} [{i}]")
    else:
        assert _same_bits(ref, got), f"{sb.case_id(b)} n {n}{what}: differs from the NT = 0 build"


# ---- ew_kernel, muladd_kernel ----------------------------------------------------------------------------------------------------------
def _ew_case(op, dtype, off, n, rng):
    """One launch of ``op`` on operands ``off`` elements into their allocations, one sentinel before (off = 1) and GUARD behind each;
    returns (the output allocation, the largest error over its bound)."""
    import torch

    ops, lib = pkg("operators"), pkg("_lib")
    eps = float(np.finfo(dtype).eps)
    alpha = float(dtype(0.37))
    a = rng.standard_normal(n).astype(dtype)
    y = (2.0 + rng.random(n)).astype(dtype)  # the divisor and the in-place operand: [2, 3)

    def dev(values):
        buf = torch.full((n + off + GUARD,), SENTINEL, dtype=lib.torch_dtype(dtype), device="cuda")
        buf[off:off + n].copy_(torch.from_numpy(values))
        assert buf.data_ptr() % 256 == 0
        return buf

    ba, by, bo = dev(a), dev(y), dev(np.full(n, 3.5, dtype))
    va, vy, vo = (t[off:off + n] for t in (ba, by, bo))
    wider = np.longdouble if dtype == np.float64 else np.float64  # (an fp64 reference of an fp64 kernel would carry the error it is to measure)
    assert np.finfo(wider).nmant > np.finfo(dtype).nmant + 8, "the reference type is no wider than the kernel's"
    a64, y64 = a.astype(wider), y.astype(wider)
    exact = None
    if op == "axpy":
        ops.axpy.launch(alpha, va, vy)
        out, ref, bound = by, alpha * a64 + y64, eps * (np.abs(alpha * a64) + np.abs(y64))
    elif op == "muladd":
        fn = getattr(lib.load(), f"fus_muladd_{'f64' if dtype == np.float64 else 'f32'}")
        lib.check(fn(va.data_ptr(), vy.data_ptr(), vo.data_ptr(), n, lib.stream_ptr()), "muladd")  # out += a * y
        out, ref, bound = bo, a64 * y64 + 3.5, eps * (np.abs(a64 * y64) + 3.5)
    elif op == "scale":
        ops.scale.launch(alpha, va, vo)
        out, ref = bo, alpha * a64
    elif op == "copy":
        ops.copy.launch(va, vo)
        out, exact = bo, a
    elif op == "fill":
        ops.fill.launch(alpha, vo)
        out, exact = bo, np.full(n, alpha, dtype)
    elif op == "divide":
        ops.pointwise_divide.launch(va, vy, vo)
        out, ref = bo, a64 / y64
    else:
        ops.square.launch(va, vo)
        out, ref = bo, a64 * a64
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[:off] == SENTINEL) and np.all(got[off + n:] == SENTINEL), f"{op}: written outside the operand"
    for buf, values in ((ba, a), (by, y)):  # the inputs keep their bits
        if buf is not out:
            assert _same_bits(buf.cpu().numpy()[off:off + n], values), f"{op}: an input changed"
    if exact is not None:
        assert _same_bits(got[off:off + n], exact), f"{op}: not bitwise"
        return got, 0.0
    if op in ("scale", "divide", "square"):
        bound = eps * np.abs(ref)
    err = np.abs(got[off:off + n].astype(wider) - ref)
    ratio = float(np.max(err / bound))
    assert np.all(err <= bound), f"{op} n {n} offset {off}: {ratio:.3f} of the bound"
    return got, ratio


@pytest.mark.parametrize("dtype", sb.DTYPES)
@pytest.mark.parametrize("op", list(sb.EW_OPS) + ["muladd"])
def test_ew_and_muladd_builds(gpu, op, dtype):
    builds = _builds("muladd_kernel", dtype) if op == "muladd" else _builds("ew_kernel", dtype, op=op)
    assert len(builds) == 6
    for W, group in _by_width(builds).items():
        for n in (SMALL, sb.sweep_size(group[0])):
            cached = None
            for b in group:
                s = sb.steer(b)
                with _tuned(s["mode"]):
                    got, ratio = _ew_case(op, NP[dtype], s["offset"], n, np.random.default_rng(7 * n + W))
                _log(b, n, op, ratio)
                if b.NT == 0:
                    cached = got
                else:
                    _assert_same(cached, got, b, n)


# ---- the RK4 stage kernels -------------------------------------------------------------------------------------------------------------
RK4 = {"stage": "rk4_stage_kernel", "nl2": "rk4_stage_nl2_kernel", "nl": "rk4_stage_nl_kernel"}


def _rk4_sweep_kinds(entry, b):
    """The kinds build ``b`` runs at the sweep size: the builds of ``rk4_stage_kernel`` (12) take kinds 0 .. 7 in turn; the 6 of
    ``rk4_stage_nl2_kernel`` and the 2 of ``rk4_stage_nl_kernel`` are fewer than their kinds, so the first ones take a second kind."""
    i = _index(b)
    if entry == "stage":
        return [i % 8]
    return [k for k in (i, i + 6) if k < 8] if entry == "nl2" else [i, i + 2]


def _rk4_runs(entry, b, n):
    """(kind, entry point) of every launch of build ``b`` at size ``n``: at the small size every kind (and nl2 without and with ``w``)."""
    if n == SMALL:
        return [(k, e) for k in range(4 if entry == "nl" else 8) for e in (("nl2", "nl2_w") if entry == "nl2" else (entry,))]
    return [(k, "nl2_w" if entry == "nl2" and _index(b) % 2 else entry) for k in _rk4_sweep_kinds(entry, b)]


# (only rk4_stage_kernel has a wide build)
RK4_CASES = [(e, d, w) for e in RK4 for d in sb.DTYPES for w in ((False, True) if e == "stage" else (False,))]


@pytest.mark.parametrize("entry,dtype,wide", RK4_CASES, ids=[f"{e}-{d}-{'wide' if w else 'scalar'}" for e, d, w in RK4_CASES])
def test_rk4_stage_builds(gpu, entry, dtype, wide):
    """``_rk4_table_case`` of tests/test_operators_gpu.py: 1e-14 / 1e-6 of the output's largest magnitude, b zero over [0, n), untouched
    vectors bitwise, also outside the operand.  Small: 1027 dofs, 1022 owned, every kind (nl2 without and with ``w``)."""
    import test_operators_gpu as t_ops

    groups = _by_width(_builds(RK4[entry], dtype))
    assert max(groups) == (16 // sb.ITEMSIZE[dtype] if entry == "stage" else 1)
    group = groups[max(groups) if wide else 1]
    W = group[0].W
    for n in (SMALL, sb.sweep_size(group[0])):
        cached = {}
        for b in group:
            s = sb.steer(b)
            runs = _rk4_runs(entry, b, n)
            # the NT = 0 build also runs what the others of its width run, for the bitwise comparison
            baseline = [r for c in group[1:] for r in _rk4_runs(entry, c, n) if r not in runs] if b.NT == 0 else []
            for kind, e in runs + baseline:
                figures = {}
                with _tuned(s["mode"]):
                    got = t_ops._rk4_table_case(NP[dtype], e, n, n - 5, s["offset"], kind, np.random.default_rng(100 * kind + W), figures)
                if (kind, e) in runs:
                    _log(b, n, f"kind {kind} {e}", max(figures.values()))
                if b.NT == 0:
                    cached[kind, e] = got
                else:
                    _assert_same(cached[kind, e], got, b, n, f" kind {kind} {e}")


def test_rk4_sweep_kinds_cover_every_kind():
    for entry, kernel in RK4.items():
        kinds = {k for b in sb.MATRIX if b.kernel == kernel for k in _rk4_sweep_kinds(entry, b)}
        assert kinds == set(range(4 if entry == "nl" else 8)), entry
    ws = {e for b in sb.MATRIX if b.kernel == RK4["nl2"] for _, e in _rk4_runs("nl2", b, 0)}
    assert ws == {"nl2", "nl2_w"}


# ---- bioheat_stage_kernel --------------------------------------------------------------------------------------------------------------
# the sweep size's rotation, by the build's position among the six of its (type, LAST): (kind, pr, s, cem43, tmax, init)
BIOHEAT_STAGES = [(0, True, True), (1, False, True), (0, True, False), (1, True, True), (1, False, False), (0, False, False)]
BIOHEAT_LAST = [(True, True, True, True, False), (False, True, True, False, True), (True, False, False, True, True), (True, True, True, True, True),
                (False, False, True, True, False), (True, True, False, False, False)]


def _bioheat_runs(b, n, position):
    """The argument tuples (kind, pr, s, cem43, tmax, init) of build ``b`` at size ``n``: at the small size all that
    ``test_stage_kernel_against_numpy`` runs for the build's kinds, at the sweep size one."""
    last = dict(b.flags)["LAST"]
    if n != 1003:
        if last:
            return [(2,) + BIOHEAT_LAST[position]]
        kind, pr, s = BIOHEAT_STAGES[position]
        return [(kind, pr, s, False, False, False)]
    dose = [(c, t, i) for c in (False, True) for t in (False, True) for i in (False, True)] if last else [(False, False, False)]
    return [(kind, pr, s) + d for kind in ((2,) if last else (0, 1)) for pr in (False, True) for s in (False, True) for d in dose]


@pytest.mark.parametrize("wide", [False, True], ids=["scalar", "wide"])
@pytest.mark.parametrize("last", [False, True], ids=["stages", "LAST"])
@pytest.mark.parametrize("dtype", sb.DTYPES)
def test_bioheat_stage_builds(gpu, dtype, last, wide):
    """``_stage_case`` of tests/test_bioheat_gpu.py: 8 eps sum|terms|, both dose bounds, b zero over [0, ntotal), the rest bitwise.
    Small: ntotal 1003, nlocal 997; sweep: nlocal = ntotal - 5."""
    import test_bioheat_gpu as t_bio

    groups = _by_width(_builds("bioheat_stage_kernel", dtype, LAST=last))
    W = max(groups) if wide else 1
    group = groups[W]
    for n, nlocal in ((1003, 997), (sb.sweep_size(group[0]), sb.sweep_size(group[0]) - 5)):
        cached = {}
        for b in group:
            s = sb.steer(b)
            runs = _bioheat_runs(b, n, 3 * wide + b.NT)
            baseline = [r for c in group[1:] for r in _bioheat_runs(c, n, 3 * wide + c.NT) if r not in runs] if b.NT == 0 else []
            for run in runs + baseline:
                figures = {}
                with _tuned(s["mode"]):
                    got = t_bio._stage_case(run[0], NP[dtype], s["offset"], n, nlocal, *run[1:], seed=run[0] + 3 * s["offset"], figures=figures)
                if run in runs and n != 1003:
                    _log(b, n, "kind %d pr %d s %d cem43 %d tmax %d init %d" % run, max(figures.values()))
                if b.NT == 0:
                    cached[run] = got
                else:
                    _assert_same(cached[run], got, b, n, f" {run}")
            if n == 1003:
                print(f"stream_builds {sb.case_id(b)} n 1003: {len(runs)} launches within their bounds")


def test_bioheat_sweep_rotation_covers_every_kind_and_operand():
    assert {k for k, _, _ in BIOHEAT_STAGES} == {0, 1}
    for column in list(zip(*BIOHEAT_STAGES))[1:] + list(zip(*BIOHEAT_LAST)):
        assert set(column) == {False, True}


# ---- relax_stage_kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["scalar", "wide"])
@pytest.mark.parametrize("nr", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", sb.DTYPES)
def test_relax_stage_builds(gpu, dtype, nr, wide):
    """``_relax_stage_case`` of tests/test_relaxation_gpu.py: 16 eps max(1, max|ref|), padding and unwritten arrays bitwise, the written /
    not-written check.  Small: 1027 owned dofs in every kind; sweep: one kind, rotating over (type, NR, width)."""
    import test_relaxation_gpu as t_relax

    groups = _by_width(_builds("relax_stage_kernel", dtype, NR=nr))
    group = groups[max(groups) if wide else 1]
    sweep_kind = (nr + int(wide) + sb.DTYPES.index(dtype)) % 3
    for n, kinds in ((SMALL, (0, 1, 2)), (sb.sweep_size(group[0]), (sweep_kind,))):
        cached = None
        for nt in (0, 1, 2):
            pair = [b for b in group if b.NT == nt]  # scalar and per-dof weights
            assert sorted(dict(b.flags)["PERDOF"] for b in pair) == [False, True]
            s = sb.steer(pair[0])
            assert all(sb.steer(b)["offset"] == s["offset"] and sb.steer(b)["odd_stride"] == s["odd_stride"] for b in pair)
            figures = {}
            got = t_relax._relax_stage_case(NP[dtype], nr, n, offsets=(s["offset"],), mode=s["mode"], perdofs=(False, True), kinds=kinds,
                                            odd_stride=s["odd_stride"], figures=figures)
            for b in pair:
                perdof = dict(b.flags)["PERDOF"]
                for kind in kinds:
                    _log(b, n, f"kind {kind}", figures[s["offset"], perdof, kind])
                    if nt:
                        _assert_same(cached[s["offset"], perdof, kind], got[s["offset"], perdof, kind], b, n, f" kind {kind}")
            if nt == 0:
                cached = got


def test_relax_sweep_rotation_covers_every_kind():
    assert {(nr + wide + d) % 3 for nr in (1, 2, 3, 4) for wide in (0, 1) for d in (0, 1)} == {0, 1, 2}


# ---- field_accumulate_kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["scalar", "wide"])
@pytest.mark.parametrize("H", range(5))
@pytest.mark.parametrize("dtype", sb.DTYPES)
def test_field_accumulate_builds(gpu, dtype, H, wide):
    """``_kernel_case`` of tests/test_field_monitor_gpu.py with H in 0 .. 4: extrema bitwise, sums within 2 N 2^-52 sum|terms|, guards and
    switched-off outputs at the sentinel.  Small: 1027 dofs, every output set, windows of 5 and 3 records -- of these the sets with
    "harm" run the H build, the others the H = 0 build (the entry point is called with H = 0 where hre / him are off).  Sweep: one output
    set per build (``_monitor_sweep_sets``: with "harm" for H > 0, so that the launch IS the H build), one window of two records
    (``init``, then accumulate).  The helper reports the H of every launch; it is asserted."""
    import test_field_monitor_gpu as t_mon

    groups = _by_width(_builds("field_accumulate_kernel", dtype, H=H))
    group = groups[max(groups) if wide else 1]
    sweep_set = lambda b: _monitor_sweep_set(H, wide, b.NT)  # noqa: E731
    for n in (SMALL, sb.sweep_size(group[0])):
        cached = {}
        for b in group:
            s = sb.steer(b)
            assert s["odd_stride"] == bool(s["offset"])  # (_Buffers: rows an odd number of doubles apart where the operands are shifted)
            if n == SMALL:
                runs = [None]  # every output set
            else:
                runs = [sweep_set(b)] + ([sweep_set(c) for c in group[1:] if sweep_set(c) != sweep_set(b)] if b.NT == 0 else [])
            for i, outs in enumerate(runs):
                collect, figures, launched = [], [], []
                with _tuned(s["mode"]):
                    if outs is None:
                        t_mon._kernel_case(NP[dtype], H, s["offset"], sizes=(n,), collect=collect, figures=figures, launched=launched)
                        assert set(launched) == {0, H} and launched.count(H) == 8 * (2 if H else 4)  # (8 records per set)
                    else:
                        t_mon._kernel_case(NP[dtype], H, s["offset"], sizes=(n,), sets=(outs,), windows=(2,), collect=collect, figures=figures,
                                           launched=launched)
                        assert launched == [H, H], f"{sb.case_id(b)} n {n} {outs}: launched with H = {launched}"
                if i == 0:
                    _log(b, n, "all sets" if outs is None else "+".join(outs), max(figures, default=0.0))
                if b.NT == 0:
                    cached[outs] = collect
                else:
                    _assert_same(cached[outs], collect, b, n, f" {outs}")


def _monitor_sweep_sets(H):
    """The output sets of the sweep size.  The entry point is called with the H of hre / him only where they are on, so every set of an
    H > 0 build contains "harm": without it the launch would run the H = 0 build."""
    if H == 0:
        return [("peak",), ("usq",), ("vsq",), ("peak", "usq", "vsq")]
    return [("harm",), ("peak", "harm"), ("usq", "harm"), ("vsq", "harm"), ("peak", "usq", "vsq", "harm")]


def _monitor_sweep_set(H, wide, nt):
    sets = _monitor_sweep_sets(H)
    return sets[(H + 3 * int(wide) + nt) % len(sets)]


def test_monitor_sweep_rotation_covers_every_output_set():
    for H in range(5):
        used = {_monitor_sweep_set(H, wide, nt) for wide in (0, 1) for nt in (0, 1, 2)}
        assert all(("harm" in outs) == (H > 0) for outs in used) and len(used) >= 4
        assert {o for outs in used for o in outs} == {"peak", "usq", "vsq"} | ({"harm"} if H else set()), H


# ---- sponge_terms_kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sb.DTYPES)
def test_sponge_terms_builds(gpu, dtype):
    """``_sponge_case`` of tests/test_sponge_gpu.py.  Small: the lists and offsets of ``test_sponge_terms_kernel``; sweep: 2048 x 256 + 778
    ascending distinct indices into a vector three times as long.  The indices are distinct: the float atomics add once per entry of y, and
    the NT builds (non-temporal loads of the list) give the cached build's bits."""
    import test_sponge_gpu as t_sponge

    group = _by_width(_builds("sponge_terms_kernel", dtype))[1]
    n_sweep = sb.sweep_size(group[0])
    assert n_sweep == 2048 * 256 + 778
    idx_sweep = np.sort(np.random.default_rng(5).choice(3 * n_sweep, size=n_sweep, replace=False)).astype(np.int32)
    cached = {}
    for b in group:
        s = sb.steer(b)
        for n, offset, nd, idx in [(n, off, 3000, None) for n in (0, 1, 257, 1000) for off in (0, 1)] + [(n_sweep, 0, 3 * n_sweep, idx_sweep)]:
            figures = {}
            with _tuned(s["mode"]):
                got = t_sponge._sponge_case(NP[dtype], n, offset, nd=nd, idx=idx, figures=figures)
            if n in (1000, n_sweep):
                _log(b, n, f"offset {offset}", figures["list"])
            if b.NT == 0:
                cached[n, offset] = got
            else:
                _assert_same(cached[n, offset], got, b, n)


# ---- mass_gather_kernel ----------------------------------------------------------------------------------------------------------------
def _gather_dofmap(rng, nrows, dense, N):
    """A generator of its own, not that of ``test_mass_gather_random_dofmaps`` (whose number of touched dofs is random, where the sweep
    case needs an exact number of row blocks): it keeps that generator's features -- dofs repeated inside an entity, three hot dofs with
    80 more entries each, a range of dofs nobody touches (sparse) -- with exactly ``nrows`` touched dofs: 0 .. nrows - 1 (dense), or with a dead zone in
    the middle and an untouched end (sparse).  Returns (dofmap [nent, N] int32, the length of the dof vector)."""
    if dense:
        touched, nd = np.arange(nrows), nrows
    else:
        dead = nrows // 10 + 1
        touched, nd = np.concatenate((np.arange(nrows // 3), np.arange(nrows // 3 + dead, nrows + dead))), nrows + dead + 37
    nent = -(-(2 * nrows + 240) // N)
    extra = rng.choice(touched, size=nent * N - nrows)
    for k, h in enumerate(rng.choice(touched, size=3, replace=False)):
        extra[80 * k: 80 * (k + 1)] = h
    flat = np.concatenate((touched, extra))
    rng.shuffle(flat)
    return flat.reshape(nent, N).astype(np.int32), nd


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("dtype", sb.DTYPES)
def test_mass_gather_builds(gpu, dtype, R):
    """Against ``np.add.at`` in fp64 at tol x max_len (1e-13 / 2e-5) of ``test_mass_gather_random_dofmaps``; the static companion bitwise
    the default apply; NT = 1 (mode 2) bitwise NT = 0 (mode 0): every row is summed by one thread in ascending entry order.  Small: 997
    touched dofs; sweep: ``stream_builds.gather_rows``.  Untouched dofs and the guard behind y keep their bits."""
    import torch

    _, lib = gpu
    L = lib.load()
    dt, sfx = NP[dtype], dtype
    tol = 1e-13 if dtype == "f64" else 2e-5
    builds = _builds("mass_gather_kernel", dtype, R=R)
    assert len(builds) == 8
    for dense in (True, False):
        for nrows, N in ((997, 8), (sb.gather_rows(R), 27)):
            rng = np.random.default_rng(1000 * R + 10 * dense + (nrows == 997))
            dm, nd = _gather_dofmap(rng, nrows, dense, N)
            nent = dm.shape[0]
            counts = np.bincount(dm.reshape(-1), minlength=nd)
            assert int((counts > 0).sum()) == nrows and 80 < counts.max() <= 250
            x, c, dj, y0 = rng.standard_normal(nd), rng.standard_normal(nent), rng.uniform(0.5, 1.5, (nent, N)), rng.standard_normal(nd)
            x, c, dj, y0 = (a.astype(dt) for a in (x, c, dj, y0))
            ref = y0.astype(np.float64)
            np.add.at(ref, dm.reshape(-1), (x.astype(np.float64)[dm] * dj.astype(np.float64) * c.astype(np.float64)[:, None]).reshape(-1))
            dm_d, xd, cd, djd = (torch.from_numpy(a).cuda() for a in (dm, x, c, dj))
            nbytes = int(L.fus_mass_gather_plan_bytes(N, nent, nd))
            sbytes = int(L.fus_mass_gather_static_bytes(N, nent, dt().itemsize))
            ws, sws = (torch.empty(k, dtype=torch.uint8, device="cuda") for k in (nbytes, sbytes))
            assert L.fus_mass_gather_plan_build(dm_d.data_ptr(), N, nent, nd, ws.data_ptr(), nbytes, None) == 0
            try:
                info = (ctypes.c_int64 * 4)()
                assert L.fus_mass_gather_plan_info(ws.data_ptr(), info) == 0
                assert (info[0], info[1], info[2]) == (nrows, int(dense), int(counts.max()))
                assert getattr(L, f"fus_mass_gather_static_build_{sfx}")(ws.data_ptr(), djd.data_ptr(), sws.data_ptr(), sbytes, None) == 0
                cached = None
                for nt in (0, 1):
                    default, static = ([b for b in builds if b.NT == nt and dict(b.flags) == dict(DENSE=dense, R=R, STATIC=st)] for st in (False, True))
                    assert len(default) == len(static) == 1
                    s = sb.steer(default[0])
                    assert s["mass_variant"] == R and sb.steer(static[0])["mode"] == s["mode"]
                    ybuf, ysbuf = (torch.full((nd + GUARD,), SENTINEL, dtype=lib.torch_dtype(dt), device="cuda") for _ in range(2))
                    for buf in (ybuf, ysbuf):
                        buf[:nd].copy_(torch.from_numpy(y0))
                    with _tuned(s["mode"], mass_variant=R):
                        assert getattr(L, f"fus_mass_apply_gather_{sfx}")(xd.data_ptr(), cd.data_ptr(), ybuf.data_ptr(), djd.data_ptr(), ws.data_ptr(), N, nent, None) == 0
                        assert getattr(L, f"fus_mass_apply_gather_static_{sfx}")(xd.data_ptr(), cd.data_ptr(), ysbuf.data_ptr(), ws.data_ptr(), sws.data_ptr(), N, nent, None) == 0
                        torch.cuda.synchronize()
                    y, ys = ybuf.cpu().numpy(), ysbuf.cpu().numpy()
                    assert np.all(y[nd:] == SENTINEL) and np.all(ys[nd:] == SENTINEL), "written behind y"
                    assert _same_bits(y[:nd][counts == 0], y0[counts == 0]), "an untouched dof changed"
                    err = np.abs(y[:nd].astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1.0)
                    _log(default[0], nrows, "dense" if dense else "sparse", err / (tol * int(counts.max())))
                    assert err < tol * int(counts.max())
                    assert _same_bits(ys, y), f"{sb.case_id(static[0])} n {nrows}: the static companion differs from the default apply"
                    _log(static[0], nrows, "dense" if dense else "sparse", err / (tol * int(counts.max())))
                    if nt == 0:
                        cached = y
                    else:
                        _assert_same(cached, y, default[0], nrows)
            finally:
                L.fus_plan_release(sws.data_ptr())
                L.fus_plan_release(ws.data_ptr())


# ---- (c) the piece seam ----------------------------------------------------------------------------------------------------------------
SEAM = sb.LAUNCH_DOFS
CHUNK = 1 << 23


def _need_memory():
    import torch

    free = torch.cuda.mem_get_info()[0]
    if free < 24 << 30:
        pytest.skip(f"the seam cases need 24 GB of free device memory, torch.cuda.mem_get_info() reports {free / 2**30:.1f} GB")


class _Drawn:
    """Device vectors drawn chunk by chunk from seeded generators, so that any chunk can be drawn again after a launch has overwritten it:
    ``fill(name, t, lo, hi)`` fills ``t`` with uniform values (``signed``: of either sign) and ``again(name, start, stop)`` returns what
    ``fill`` wrote to t[start:stop] (start a multiple of CHUNK)."""

    def __init__(self, seed):
        import torch

        self.g, self.seed, self.spec = torch.Generator(device="cuda"), seed, {}

    def _chunk(self, name, k, size):
        import torch

        lo, hi, signed, dtype, order = self.spec[name]
        self.g.manual_seed((self.seed * 64 + order) * 4096 + k)
        t = torch.empty(size, dtype=dtype, device="cuda").uniform_(lo, hi, generator=self.g)
        if signed:
            t = torch.where(torch.empty(size, dtype=torch.float32, device="cuda").uniform_(0, 1, generator=self.g) < 0.5, -t, t)
        return t

    def fill(self, name, t, lo, hi, signed=False):
        self.spec[name] = (lo, hi, signed, t.dtype, len(self.spec))
        for k, start in enumerate(range(0, t.numel(), CHUNK)):
            stop = min(start + CHUNK, t.numel())
            t[start:stop].copy_(self._chunk(name, k, stop - start))
        return t

    def again(self, name, start, stop, total):
        """t[start:stop] as drawn, of a vector of ``total`` entries (start a multiple of CHUNK, stop inside the same chunk)."""
        assert start % CHUNK == 0 and stop <= min(start + CHUNK, total)
        return self._chunk(name, start // CHUNK, min(start + CHUNK, total) - start)[: stop - start]


def _guarded(n, dtype):
    """(the allocation, its first ``n`` entries): GUARD sentinel entries behind the vector."""
    import torch

    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf[:n]


def _guard_kept(buf, n):
    return bool((buf[n:] == SENTINEL).all().item())


def test_piece_seam_field_accumulate(gpu):
    """fus_field_accumulate_f32 on 2^27 + 1029 dofs: two launches per record, the second of 1029 dofs from every base + 2^27.  Peak, usq
    and H = 1, two records (``init``, then accumulate), aligned.  Extrema bitwise; sums within 2 N 2^-52 sum|terms| of the same sequence
    in torch fp64; guards at the sentinel."""
    import torch

    _need_memory()
    _, lib = gpu
    n, records, eps = SEAM + 1029, 2, 2.0**-52
    stride = n + GUARD + ((n + GUARD) & 1)  # (one row: the stride only has to be even for the wide build)
    assert stride % 2 == 0 and n > sb.LAUNCH_DOFS
    drawn = _Drawn(31)
    us = [drawn.fill(f"u{k}", torch.empty(n, dtype=torch.float32, device="cuda"), -10.0, 10.0) for k in range(records)]
    (bmax, pmax), (bmin, pmin) = _guarded(n, torch.float32), _guarded(n, torch.float32)
    (busq, usq), (bre, hre), (bim, him) = (_guarded(n, torch.float64) for _ in range(3))
    coefs = np.random.default_rng(31).uniform(-1.0, 1.0, (records, 2))
    for k in range(records):
        cd = torch.from_numpy(coefs[k]).cuda()
        rc = lib.load().fus_field_accumulate_f32(us[k].data_ptr(), None, n, pmax.data_ptr(), pmin.data_ptr(), usq.data_ptr(), None, hre.data_ptr(),
                                                 him.data_ptr(), stride, cd.data_ptr(), 1, int(k == 0), lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
    extrema, worst = True, 0.0
    for start in range(0, n, CHUNK):
        sl = slice(start, min(start + CHUNK, n))
        a, b = us[0][sl], us[1][sl]
        extrema = extrema and torch.equal(pmax[sl], torch.maximum(a, b)) and torch.equal(pmin[sl], torch.minimum(a, b))
        a, b = a.double(), b.double()
        for got, t0, t1 in ((usq, a * a, b * b), (hre, a * coefs[0, 0], b * coefs[1, 0]), (him, a * coefs[0, 1], b * coefs[1, 1])):
            bound = 2 * records * eps * (t0.abs() + t1.abs())
            worst = max(worst, float(((got[sl] - (t0 + t1)).abs() / bound).max().item()))
    print(f"stream_builds seam field_accumulate f32 n {n}: max err / bound {worst:.3f}")
    assert extrema, "pmax / pmin are not bitwise the extrema"
    assert worst <= 1.0
    assert all(_guard_kept(buf, n) for buf in (bmax, bmin, busq, bre, bim))
    assert all(torch.equal(us[k][:CHUNK], drawn.again(f"u{k}", 0, CHUNK, n)) for k in range(records)), "u changed"


def test_piece_seam_bioheat_stage(gpu):
    """fus_bioheat_stage_f32, LAST with pr, s, cem43 and tmax (updated: init = 0), nlocal = 2^27 + 5 of ntotal = 2^27 + 1029: the owned range
    ends one dof into the second piece's scalar tail and the ghost block follows.  ``_stage_case``'s checks in torch fp64: T0 within 8 eps
    sum|terms|, both dose bounds, tmax bitwise the maximum, b zero over [0, ntotal), ghosts, guards and inputs bitwise."""
    import torch

    _need_memory()
    _, lib = gpu
    nlocal, ntotal = SEAM + 5, SEAM + 1029
    eps, eps64, ln4 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps), math.log(4.0)
    dt = 0.37
    bw, aw, gate, Ta = (float(np.float32(x)) for x in (dt / 6.0, dt / 2.0, 0.7, 37.0))
    drawn = _Drawn(32)
    ranges = dict(minv=(0.5, 2.0), b=(-3.0, 3.0), T0=(36.0, 50.0), Tn=(36.0, 50.0), acc=(36.0, 50.0), pr=(0.0, 0.5), s=(0.0, 4.0), tmax=(36.0, 50.0),
                  cem43=(0.0, 30.0))
    size = {k: nlocal if k in ("tmax", "cem43") else ntotal for k in ranges}
    bufs, v = {}, {}
    for k, (lo, hi) in ranges.items():
        bufs[k], v[k] = _guarded(size[k], torch.float64 if k == "cem43" else torch.float32)
        drawn.fill(k, v[k], lo, hi)
    p = lambda k: v[k].data_ptr()  # noqa: E731
    rc = lib.load().fus_bioheat_stage_f32(bw, aw, 2, gate, Ta, dt, p("minv"), p("pr"), p("s"), p("b"), p("T0"), p("Tn"), p("acc"), p("cem43"), p("tmax"), 0,
                                          nlocal, ntotal, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    inc = lambda T: dt / 60.0 * torch.exp2((43.0 - T) * torch.where(T >= 43.0, -1.0, -2.0))  # noqa: E731
    worst = dict(T0=0.0, cem43_ref=0.0, cem43_own=0.0)
    kept, tmax_ok = True, True
    for start in range(0, ntotal, CHUNK):
        stop = min(start + CHUNK, ntotal)
        own = max(min(stop, nlocal) - start, 0)  # owned dofs of this chunk
        was = {k: drawn.again(k, start, min(stop, size[k]), size[k]) for k in ranges if start < size[k]}
        for k in ("minv", "Tn", "acc", "pr", "s"):
            kept = kept and torch.equal(v[k][start:stop], was[k])
        kept = kept and torch.equal(v["T0"][start + own:stop], was["T0"][own:])  # the ghost entries
        if own == 0:
            continue
        o = slice(start, start + own)
        minv, b, Tn, acc, pr, s = (was[k][:own].double() for k in ("minv", "b", "Tn", "acc", "pr", "s"))
        k_ = minv * b - pr * (Tn - Ta) + gate * s
        ka = (minv * b).abs() + (pr * Tn).abs() + (pr * Ta).abs() + (gate * s).abs()
        ref, terms = acc + bw * k_, acc.abs() + abs(bw) * ka
        new = v["T0"][o]
        worst["T0"] = max(worst["T0"], float(((new.double() - ref).abs() / (8 * eps * terms)).max().item()))
        tmax_ok = tmax_ok and torch.equal(v["tmax"][o], torch.maximum(was["tmax"][:own], new))
        cem_ref, cem_own = was["cem43"][:own] + inc(ref), was["cem43"][:own] + inc(new.double())
        dT = (new.double() - ref).abs()
        worst["cem43_ref"] = max(worst["cem43_ref"], float(((v["cem43"][o] - cem_ref).abs() / ((ln4 * dT + 4 * eps) * cem_ref)).max().item()))
        worst["cem43_own"] = max(worst["cem43_own"], float(((v["cem43"][o] - cem_own).abs() / (4 * eps64 * cem_own)).max().item()))
    print("stream_builds seam bioheat_stage f32 LAST nlocal %d ntotal %d: max err / bound T0 %.3f cem43 (reference) %.3f cem43 (own T0) %.3f"
          % (nlocal, ntotal, worst["T0"], worst["cem43_ref"], worst["cem43_own"]))
    assert not bool(v["b"].any().item()), "b must be zero over [0, ntotal)"
    assert kept, "an input or a ghost entry of T0 changed"
    assert tmax_ok, "tmax is not bitwise max(tmax, T0)"
    assert all(w <= 1.0 for w in worst.values()), worst
    assert all(_guard_kept(bufs[k], size[k]) for k in ranges)


def test_piece_seam_relax_stage(gpu):
    """fus_relax_stage_f32, NR = 2, per-dof weights, MIDDLE, nlocal = 2^27 + 1029, rows nlocal + 3 rounded up to 4 apart: rows and pieces
    together.  ``_relax_stage_case``'s checks in torch fp64: 16 eps max(1, max|ref|), the padding of every row, x0, u_base and vn bitwise,
    xn and acc written."""
    import torch

    _need_memory()
    ops, _ = gpu
    nr, nlocal = 2, SEAM + 1029
    stride = -(-(nlocal + 3) // 4) * 4
    eps = float(np.finfo(np.float32).eps)
    tau = np.array([0.7, 1.3])
    itau = (1.0 / tau).astype(np.float32).astype(np.float64)
    bw, aw, aw_u = (float(np.float32(x)) for x in (0.31, 0.47, 0.23))
    drawn = _Drawn(33)
    state = {}
    for name in ("x0", "xn", "acc", "kd"):
        t = torch.empty(nr * stride, dtype=torch.float32, device="cuda")
        assert t.data_ptr() % 256 == 0
        for nu in range(nr):
            drawn.fill(f"{name}{nu}", t[nu * stride:(nu + 1) * stride], *((0.2, 1.0, False) if name == "kd" else (0.5, 2.0, True)))
        state[name] = t.view(nr, stride)
    ub, vn, ur = (drawn.fill(k, torch.empty(nlocal + 2, dtype=torch.float32, device="cuda"), 0.5, 2.0) for k in ("ub", "vn", "ur"))
    ops.relax_stage(bw, aw, aw_u, 1, tau, state["kd"], state["x0"], state["xn"], state["acc"], ub, vn, ur, nlocal)
    torch.cuda.synchronize()
    err, top = dict(xn=0.0, acc=0.0, ur=0.0), dict(xn=0.0, acc=0.0, ur=0.0)
    kept, written = True, dict(xn=False, acc=False)
    for start in range(0, stride, CHUNK):
        stop = min(start + CHUNK, stride)
        own = max(min(stop, nlocal) - start, 0)
        o = slice(start, start + own)
        v_was = drawn.again("vn", start, min(stop, nlocal + 2), nlocal + 2) if start < nlocal + 2 else None
        if v_was is not None:
            u_was = drawn.again("ub", start, min(stop, nlocal + 2), nlocal + 2)
            kept = kept and torch.equal(vn[start:stop], v_was) and torch.equal(ub[start:stop], u_was)
            kept = kept and torch.equal(ur[start + own:stop], drawn.again("ur", start, min(stop, nlocal + 2), nlocal + 2)[own:])  # past nlocal
            ur_ref = u_was[:own].double() + aw_u * v_was[:own].double()
        for nu in range(nr):
            was = {k: drawn.again(f"{k}{nu}", start, stop, stride) for k in ("x0", "xn", "acc", "kd")}
            kept = kept and torch.equal(state["x0"][nu, start:stop], was["x0"]) and torch.equal(state["kd"][nu, start:stop], was["kd"])
            for k in ("xn", "acc"):  # the padding of the row
                kept = kept and torch.equal(state[k][nu, start + own:stop], was[k][own:])
            if own == 0:
                continue
            x0, xn, acc, kd = (was[k][:own].double() for k in ("x0", "xn", "acc", "kd"))
            k_ = kd * v_was[:own].double() - xn * itau[nu]
            ref = dict(acc=acc + bw * k_, xn=x0 + aw * k_)
            ur_ref = ur_ref + ref["xn"]
            for k in ("xn", "acc"):
                err[k] = max(err[k], float((state[k][nu, o].double() - ref[k]).abs().max().item()))
                top[k] = max(top[k], float(ref[k].abs().max().item()))
                written[k] = written[k] or not torch.equal(state[k][nu, o], was[k][:own])
        if own:
            err["ur"] = max(err["ur"], float((ur[o].double() - ur_ref).abs().max().item()))
            top["ur"] = max(top["ur"], float(ur_ref.abs().max().item()))
    ratios = {k: err[k] / (16 * eps * max(1.0, top[k])) for k in err}
    print("stream_builds seam relax_stage f32 NR 2 per-dof MIDDLE nlocal %d stride %d: max err / bound xn %.3f acc %.3f ur %.3f"
          % (nlocal, stride, ratios["xn"], ratios["acc"], ratios["ur"]))
    assert kept, "x0, the weights, u_base, vn, a row's padding or ur past nlocal changed"
    assert all(written.values()), written
    assert all(r <= 1.0 for r in ratios.values()), ratios
