"""Every build of tests/small_kernel_builds.py on the GPU, through the Python entry points the solvers use (the ``precompute.*_device``
functions, ``operators.facet_terms`` / ``facet_source_terms``, ``scatterer.HipHaloKernels``), at the shapes where such kernels go wrong
and at the record's sweep size, where the grid is at its cap and the grid-stride loop takes a second trip.

    geometry, facet geometry   against the longdouble model of tests/geometry_model.py, per (cell, q): at most 8 x e_cpu in the maximum
                               and in the root mean square, every family x every nq, 300 cells; the three output forms bitwise equal
    facet terms and sources    the reference and tolerance of each kernel's own test (tests/facet_cpu.py) and the per-dof bound
                               (k + 3) eps (|y0| + sum |terms|) (fp64 sources: plus the slack of two fp64 evaluations of g_e); N = (P + 1)^2 for P = 1 .. 10 (and N = 1), empty sets, both scalar
                               forms, both stage forms; dofs that only inactive, silent or out-of-table facets touch keep their bits
    halo                       pack / unpack_fwd bitwise numpy, unpack_rev within the per-dof bound, counts 0, 1, 256, 257 and the sweep;
                               untouched entries keep their bits; one pack_rev reads beyond 2^31 elements

Every output buffer carries a 256-byte guard of 0xA5 behind it, which must keep its bytes.  Every test prints ``ratio <kernel> <type>
<case> <error / bar>``: profiles/small_kernel_errors.log is those lines of one run."""

import functools

import numpy as np
import pytest

import facet_cpu
import geometry_model as gm
import small_kernel_builds as sk
import waveform_cpu
from conftest import TOL, pkg, rel_l2, rel_max

pytestmark = pytest.mark.gpu

DTYPES = {"f64": np.float64, "f32": np.float32}
GUARD, POISON = 256, 0xA5
NCELL, NFACETS = 300, 500
F0 = 0.5e6
DT_TAB, T0_TAB, T_STAGE = 2.0**-24, 5 * 2.0**-24, 40 * 2.0**-24  # the table of tests/test_waveform_sources_gpu.py: exact node times


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _td(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).to("cuda")  # a copy: the shared cases are read-only


def _guarded(init=None, shape=None, dtype=None):
    """(the allocation in bytes, a tensor view of its front): the view holds ``init`` (else every byte is 0xA5: a poisoned output) and
    256 bytes of 0xA5 stand behind it."""
    import torch

    if init is not None:
        init = np.ascontiguousarray(init)
        shape, dtype = init.shape, init.dtype
    dtype = np.dtype(dtype)
    tdt = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}[dtype]
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    raw = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 256 == 0
    view = (raw[:nbytes].view(tdt) if nbytes else raw[: dtype.itemsize].view(tdt)[:0]).view(tuple(shape))
    if init is not None and nbytes:
        view.copy_(torch.from_numpy(init))
    return raw, view


def _guard_kept(raw):
    return bool((raw[-GUARD:] == POISON).all().item())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _report(kernel, dtype, case, ratio):
    print(f"\nratio {kernel} {dtype} {case} {ratio:.3f}")  # a line of its own, also behind pytest's progress dots


# =========================================================================================================================================
# geometry_kernel, facet_geometry_kernel
@functools.lru_cache(maxsize=None)
def _geometry_case(family, nq, dtype):
    """Inputs, model and e_cpu of one (family, nq, type), computed once."""
    T = DTYPES[dtype]
    x_dofs, x_g = gm.cells(family, NCELL, T)
    dphi, w = gm.rule(nq, T)
    Gm, dm = gm.model(x_dofs, x_g, dphi, w)
    Gr, dr = gm.restate(x_dofs, x_g, dphi, w)
    case = dict(x_dofs=x_dofs, x_g=x_g, dphi=dphi, w=w, Gm=Gm, dm=dm, eG=gm.g_errors(Gr, Gm), eD=gm.det_errors(dr, dm))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _facet_case(family, nqf, dtype):
    T = DTYPES[dtype]
    x_dofs, x_g = gm.cells(family, NCELL, T)
    dphi_f, w = gm.facet_rule(nqf, T)
    bd = gm.boundary(NCELL, NFACETS)
    Fm = gm.facet_model(x_dofs, x_g, bd, dphi_f, w)
    case = dict(x_dofs=x_dofs, x_g=x_g, dphi_f=dphi_f, w=w, bd=bd, Fm=Fm, eF=gm.det_errors(gm.facet_restate(x_dofs, x_g, bd, dphi_f, w), Fm))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _run_geometry(x_dofs, x_g, dphi, w, ncell):
    """The three output forms on the same inputs -> (G, detJ) on the host, after the checks that do not need a model: every output bitwise
    equal across the forms that produce it, every guard kept."""
    import torch

    pre = pkg("precompute")
    mesh, dphi_d, w_d = (_td(x_dofs), _td(x_g)), _td(dphi), _td(w)
    nq = w.size
    out = {}
    for form in ("G+detJ", "G", "detJ"):
        rG, G = _guarded(shape=(ncell, nq, 6), dtype=x_g.dtype)
        rD, D = _guarded(shape=(ncell, nq), dtype=x_g.dtype)
        if form == "G+detJ":
            pre.compute_scaled_geometrical_factor_device(G, mesh, ncell, dphi_d, w_d, detJ=D)
        elif form == "G":
            pre.compute_scaled_geometrical_factor_device(G, mesh, ncell, dphi_d, w_d)
        else:
            pre.compute_scaled_jacobian_determinant_device(D, mesh, ncell, dphi_d, w_d)
        torch.cuda.synchronize()
        assert _guard_kept(rG) and _guard_kept(rD), form
        out[form] = (rG, rD, G, D)
    poisoned = lambda raw: bool((raw == POISON).all().item())  # noqa: E731
    assert torch.equal(out["G+detJ"][0], out["G"][0]), "G differs between the form with detJ and the form without"
    assert torch.equal(out["G+detJ"][1], out["detJ"][1]), "detJ differs between the form with G and the form without"
    assert poisoned(out["G"][1]) and poisoned(out["detJ"][0]), "an output that was not asked for was written"
    return out["G+detJ"][2], out["G+detJ"][3]


def _geometry_ratios(G, D, case, label, dtype):
    eG, eD = gm.g_errors(G, case["Gm"]), gm.det_errors(D, case["dm"])
    ratios = [eG[0] / (gm.BAR * case["eG"][0]), eG[1] / (gm.BAR * case["eG"][1]), eD[0] / (gm.BAR * case["eD"][0]), eD[1] / (gm.BAR * case["eD"][1])]
    for what, r in zip(("G-max", "G-rms", "detJ-max", "detJ-rms"), ratios):
        _report("geometry_kernel", dtype, f"{label}-{what}", r)
    return ratios


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", gm.NQ)
@pytest.mark.parametrize("family", gm.FAMILIES)
def test_geometry_against_the_model(gpu, family, nq, dtype):
    """300 cells x nq points (two workgroups at nq = 1, the second partial): G and detJ within 8 x e_cpu of the model in the maximum and
    in the root mean square; the three output forms agree bitwise."""
    case = _geometry_case(family, nq, dtype)
    G, D = _run_geometry(case["x_dofs"], case["x_g"], case["dphi"], case["w"], NCELL)
    ratios = _geometry_ratios(G.cpu().numpy(), D.cpu().numpy(), case, f"{family}-nq{nq}", dtype)
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nqf", gm.NQF)
@pytest.mark.parametrize("family", gm.FAMILIES)
def test_facet_geometry_against_the_model(gpu, family, nqf, dtype):
    """500 random (cell, local facet) pairs: unsorted, cells repeat, all six local facets."""
    import torch

    pre = pkg("precompute")
    case = _facet_case(family, nqf, dtype)
    raw, dF = _guarded(shape=(NFACETS, nqf), dtype=DTYPES[dtype])
    pre.compute_boundary_facets_scaled_jacobian_determinant_device(dF, (_td(case["x_dofs"]), _td(case["x_g"])), _td(case["bd"]), _td(case["dphi_f"]),
                                                                   _td(case["w"]))
    torch.cuda.synchronize()
    assert _guard_kept(raw)
    e = gm.det_errors(dF.cpu().numpy(), case["Fm"])
    ratios = [e[0] / (gm.BAR * case["eF"][0]), e[1] / (gm.BAR * case["eF"][1])]
    for what, r in zip(("max", "rms"), ratios):
        _report("facet_geometry_kernel", dtype, f"{family}-nqf{nqf}-{what}", r)
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES)
def test_geometry_small_sizes(gpu, dtype):
    """ncell = 0 and nfacets = 0 launch nothing: poisoned outputs keep every byte.  ncell = 1 with nq = 1 is one thread: it gives the bits
    that cell has in the 300-cell launch (whose error the model test bounds)."""
    import torch

    pre = pkg("precompute")
    T = DTYPES[dtype]
    case = _geometry_case("mirrored", 1, dtype)
    mesh, dphi_d, w_d = (_td(case["x_dofs"]), _td(case["x_g"])), _td(case["dphi"]), _td(case["w"])
    rG, G = _guarded(shape=(4, 1, 6), dtype=T)
    rD, D = _guarded(shape=(4, 1), dtype=T)
    pre.compute_scaled_geometrical_factor_device(G, mesh, 0, dphi_d, w_d, detJ=D)
    pre.compute_scaled_jacobian_determinant_device(D, mesh, 0, dphi_d, w_d)
    torch.cuda.synchronize()
    assert bool((rG == POISON).all().item()) and bool((rD == POISON).all().item())
    G300, D300 = _run_geometry(case["x_dofs"], case["x_g"], case["dphi"], case["w"], NCELL)
    for c in (0, 1, NCELL - 1):  # an ordinary cell, a mirrored one, the last
        G1, D1 = _run_geometry(case["x_dofs"][c : c + 1], case["x_g"], case["dphi"], case["w"], 1)
        assert torch.equal(G1[0], G300[c]) and torch.equal(D1[0], D300[c])
    fc = _facet_case("mirrored", 4, dtype)
    rF, dF = _guarded(shape=(3, 4), dtype=T)
    pre.compute_boundary_facets_scaled_jacobian_determinant_device(dF, (_td(fc["x_dofs"]), _td(fc["x_g"])), _td(fc["bd"][:0]), _td(fc["dphi_f"]),
                                                                   _td(fc["w"]))
    torch.cuda.synchronize()
    assert bool((rF == POISON).all().item())


@pytest.mark.parametrize("dtype", DTYPES)
def test_geometry_sweep(gpu, dtype):
    """599 298 cells x nq = 7: the grid is at its cap of 16384 workgroups and 782 threads take a second trip.  Cell c has the vertices'
    coordinates of cell c mod 997 (on vertices of its own, numbered through one permutation of all 4.8 M), so its output has the bits of
    that cell's: a wrong cell or q index anywhere, the second trip included, changes values (997 divides neither the stride nor stride /
    nq).  The first 997 cells are held to the model."""
    import torch

    b = sk.of("geometry_kernel", dtype)
    ncell, nq = b.sweep
    T = DTYPES[dtype]
    x_dofs, x_g = gm.cells("mirrored_1e-3", ncell, T, period=gm.PERIOD)
    dphi, w = gm.rule(nq, T)
    G, D = _run_geometry(x_dofs, x_g, dphi, w, ncell)
    first = torch.arange(ncell, device="cuda") % gm.PERIOD
    same_G = (G == G[first]).all(dim=2).all(dim=1)
    same_D = (D == D[first]).all(dim=1)
    bad = torch.nonzero(~(same_G & same_D)).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} cells differ from the cell they repeat, the first at (cell, q) index {int(bad[0]) * nq} of {ncell * nq}"
    head = slice(0, gm.PERIOD)
    Gm, dm = gm.model(x_dofs[head], x_g, dphi, w)
    Gr, dr = gm.restate(x_dofs[head], x_g, dphi, w)
    case = dict(Gm=Gm, dm=dm, eG=gm.g_errors(Gr, Gm), eD=gm.det_errors(dr, dm))
    ratios = _geometry_ratios(G[head].cpu().numpy(), D[head].cpu().numpy(), case, "sweep", dtype)
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES)
def test_facet_geometry_sweep(gpu, dtype):
    """466 120 facets x nqf = 9 on 4000 cells of period 997: 776 threads take a second trip.  A facet has the bits of the first facet with
    the same (cell mod 997, local facet); those 5982 representatives are held to the model."""
    import torch

    pre = pkg("precompute")
    b = sk.of("facet_geometry_kernel", dtype)
    nfacets, nqf = b.sweep
    T, ncell = DTYPES[dtype], 4000
    x_dofs, x_g = gm.cells("mirrored_1e-3", ncell, T, period=gm.PERIOD)
    dphi_f, w = gm.facet_rule(nqf, T)
    bd = gm.boundary(ncell, nfacets)
    raw, dF = _guarded(shape=(nfacets, nqf), dtype=T)
    pre.compute_boundary_facets_scaled_jacobian_determinant_device(dF, (_td(x_dofs), _td(x_g)), _td(bd), _td(dphi_f), _td(w))
    torch.cuda.synchronize()
    assert _guard_kept(raw)
    got = dF.cpu().numpy()
    _, first, inverse = np.unique((bd[:, 0] % gm.PERIOD) * 6 + bd[:, 1], return_index=True, return_inverse=True)
    assert first.size == 6 * gm.PERIOD
    bad = np.nonzero(~np.all(_bits(got) == _bits(got[first[inverse]]), axis=1))[0]
    assert bad.size == 0, f"{bad.size} facets differ from the facet they repeat, the first at (facet, q) index {bad[0] * nqf} of {nfacets * nqf}"
    Fm = gm.facet_model(x_dofs, x_g, bd[first], dphi_f, w)
    e_cpu = gm.det_errors(gm.facet_restate(x_dofs, x_g, bd[first], dphi_f, w), Fm)
    e = gm.det_errors(got[first], Fm)
    ratios = [e[0] / (gm.BAR * e_cpu[0]), e[1] / (gm.BAR * e_cpu[1])]
    for what, r in zip(("max", "rms"), ratios):
        _report("facet_geometry_kernel", dtype, f"sweep-{what}", r)
    assert max(ratios) <= 1.0, ratios


# =========================================================================================================================================
# facet_terms_kernel, facet_source_array_kernel, facet_source_wave_kernel
KINDS = {"terms": "facet_terms_kernel", "array": "facet_source_array_kernel", "wave": "facet_source_wave_kernel"}
SCALE = 7.0
# elements whose value is zero at the stage time by construction (the kernels skip their facets), and some that are live
QUIET_ELEMENTS = {"array": (0, 1, 5, 6), "wave": (0, 3, 5, 7, 9, 12, 14)}
LIVE_ELEMENTS = {"array": (2, 3, 4), "wave": (1, 2, 4)}
# the elements of the last seven facets of set A in the sweep shape whose set A exceeds the grid.  The first of them straddles the end of
# the grid; the six behind it lie wholly in the second trip and hold every reason for which a kernel skips a facet: inactive (-1), a
# time before the start (array 0, 1; wave 0: before the table), a time past the end (array 5, 6; wave 5: past the table), and, for the
# waveform kernel, a silent row (3), with live facets between them
TAIL_ELEMENTS = {"array": (2, -1, 0, 1, 5, 3, 6), "wave": (1, -1, 3, 0, 5, 2, 9)}
TAIL_REASONS = {"array": {"inactive", "before", "past", "live"}, "wave": {"inactive", "silent", "before", "past", "live"}}


def _skip_reason(kind, arr, t, e):
    """Why the kernel of ``kind`` adds nothing for a facet of element ``e`` at time ``t`` ("live": it adds), from the source's own
    parameters, not from its values."""
    if e < 0:
        return "inactive"
    s = t - arr.delay[e]
    if kind == "array":
        return "before" if s <= 0.0 else "past" if s >= arr.duration else "live"
    if arr.waveform_of_element[e] < 0:
        return "silent"
    x = (s - arr.waveform.t0) / arr.waveform.dt
    return "before" if x < 0.0 else "past" if x > arr.waveform.n_samples - 1 else "live"


def _time_cases(nt):
    """s - t0 in units of dt: before the table, on its first node, inside an interval, on an interior node, on the last node, past the
    end, inside the last interval (tests/test_waveform_sources_gpu.py)."""
    return np.array([-2.0, 0.0, 7.3, 11.0, nt - 1.0, nt - 0.5, nt - 1.25])


def _source(kind, ids, rng):
    """The source array of ``kind`` for the facets' element ids, and its stage time.

    array   23 elements, a burst of 12 periods seen at t = 14 T: the delays of elements 0 .. 6 put s = t - tau before the start, on the
            start, on the ramp, on the plateau, on the ramp down, and (5, 6) after the end; the others anywhere
    wave    16 elements on a table of 5 rows x 33 samples: element e takes time case e mod 7 (0: before the table, 5: past its end);
            elements 3 and 9 are silent (row -1)"""
    src = pkg("sources")
    if kind == "array":
        E, T = 23, 1.0 / F0
        delay = np.concatenate([[15.0 * T, 14.0 * T, 12.0 * T, 8.0 * T, 3.5 * T, 1.0 * T, 0.0], 11.0 * T * rng.random(E - 7) + T])
        arr = src.SourceArray(ids, amplitude=0.5 + rng.random(E), phase=2 * np.pi * rng.random(E) - np.pi, delay=delay, duration=12.0 * T, n_elements=E)
        return arr, 14.0 * T
    E, R, nt = 16, 5, 33
    wf = src.SampledWaveform(rng.standard_normal((R, nt)), DT_TAB, t0=T0_TAB, derivative=rng.standard_normal((R, nt)) / DT_TAB)
    row_of = rng.integers(0, R, E)
    row_of[[3, 9]] = -1
    delay = T_STAGE - (T0_TAB + _time_cases(nt)[np.arange(E) % 7] * DT_TAB)
    return src.SourceArray(ids, amplitude=0.5 + rng.random(E), delay=delay, waveform=wf, waveform_of_element=row_of, n_elements=E), T_STAGE


def _padded_constants(cB, nA):
    """cB on the device with ``nA`` other values behind it: a set B that looked its constant up by the index in BOTH sets would read
    them, inside the allocation."""
    pad = np.concatenate([cB, cB.dtype.type(3.0) + np.arange(nA, dtype=cB.dtype)])
    return _td(pad)[: cB.size]


def _facet_case_inputs(kind, dtype, N, nA, nB, ndofs, reserved, tail=0):
    """Host inputs of one facet case.  ``tail``: the last ``tail`` facets of set A (those of the second trip, in the sweep shape whose set
    A exceeds the grid) take the elements ``TAIL_ELEMENTS``."""
    T = DTYPES[dtype]
    rng = np.random.default_rng([21, list(KINDS).index(kind), T().itemsize, N, nA, nB])
    if kind == "terms":
        ids, arr, t = np.zeros(nA, dtype=np.int64), None, None
        quiet = np.zeros(nA, dtype=bool)
    else:
        E = 23 if kind == "array" else 16
        ids = rng.integers(-1, E, nA)
        if tail:
            assert tail == len(TAIL_ELEMENTS[kind])
            ids[nA - tail:] = TAIL_ELEMENTS[kind]
        arr, t = _source(kind, ids, rng)
        g, dg = arr.values(t, F0, SCALE)
        assert not np.any(g[list(QUIET_ELEMENTS[kind])]) and not np.any(dg[list(QUIET_ELEMENTS[kind])]) and np.all(g[list(LIVE_ELEMENTS[kind])] != 0)
        quiet = (ids < 0) | ((g == 0) & (dg == 0))[np.maximum(ids, 0)]
    s = facet_cpu.facet_sets(rng, T, N, nA, nB, ndofs, quiet, reserved)
    s.update(ids=ids, arr=arr, t=t, quiet=quiet, y0=rng.standard_normal(ndofs).astype(T), N=N, nA=nA, nB=nB, ndofs=ndofs, reserved=reserved, dtype=T)
    return s


def _launch(kind, s, with_c2, with_B, variant, gpu):
    """One launch of ``kind`` on the case ``s`` -> (y on the host, v1, v2): the fp64 values per facet of set A that the reference takes.

    variant   terms: "host" (s1, s2 launch arguments) / "dev" (the ``scalars=`` tensor); sources: "host" / "dev" stage block"""
    import torch

    ops = pkg("operators")
    T, nA, nB = s["dtype"], s["nA"], s["nB"]
    raw, y = _guarded(init=s["y0"])
    field = (_td(s["x"]), _padded_constants(s["cB"], nA), _td(s["dB"]), _td(s["dmB"])) if with_B else None
    c1, c2, dA, dmA = _td(s["c1"]), _td(s["c2"]) if with_c2 else None, _td(s["dA"]), _td(s["dmA"])
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    if kind == "terms":
        s1, s2 = T(0.37), T(-1.9)
        if variant == "dev":  # the launch arguments are then ignored
            ops.facet_terms(y, (c1, 123.0, c2, -456.0, dA, dmA), field, scalars=_td(np.array([s1, s2], dtype=T)))
        else:
            ops.facet_terms(y, (c1, float(s1), c2, float(s2) if with_c2 else 0.0, dA, dmA), field)
        v1, v2 = float(s1) * f64(s["c1"]), float(s2) * f64(s["c2"]) if with_c2 else None
    else:
        arr = s["arr"]
        bound = arr.bind(None, np.zeros((nA, 2), np.int32), T, gpu, frequency=F0, scale=SCALE, coeff1=c1, coeff2=c2, detJ=dA, dofmap=dmA)
        stage = bound.stage_scalars(s["t"])
        ops.facet_source_terms(y, bound, field, **(dict(stage=stage) if variant == "host" else dict(stage_dev=_td(stage))))
        g, dg = arr.values(s["t"], F0, SCALE)
        e, act = np.maximum(s["ids"], 0), s["ids"] >= 0
        v1 = np.where(act, g[e], 0.0) * f64(s["c1"])
        v2 = np.where(act, dg[e], 0.0) * f64(s["c2"]) if with_c2 else None
    torch.cuda.synchronize()
    assert _guard_kept(raw), "the guard behind y was written"
    return y.cpu().numpy(), v1, v2


def _evaluation_slack(kind, s, with_c2, v1):
    """Per dof: how far the kernel's fp64 evaluation of (g_e, dg_e) and numpy's may carry a sum apart (facet_cpu.evaluation_slack)."""
    out = np.zeros(s["ndofs"])
    if kind == "terms" or not s["nA"]:
        return out
    eg, edg = facet_cpu.evaluation_slack(s["arr"], F0, SCALE)
    e = np.maximum(s["ids"], 0)
    per_facet = eg[e] * np.abs(s["c1"].astype(np.float64)) + (edg[e] * np.abs(s["c2"].astype(np.float64)) if with_c2 else 0.0)
    live = v1 != 0
    np.add.at(out, s["dmA"][live].reshape(-1), (per_facet[live, None] * np.abs(s["dA"].astype(np.float64))[live]).reshape(-1))
    return out


def _own_reference(kind, s, with_c2, with_B, oracle_c):
    """The reference of the kernel's own test, on top of y0, and whether the whole vector meets that test's tolerance."""
    T = s["dtype"]
    field = (s["x"], s["cB"], s["dB"], s["dmB"]) if with_B else None
    if kind == "terms":
        ref = facet_cpu.terms_oracle(oracle_c, s["y0"], T(0.37), s["c1"], T(-1.9), s["c2"] if with_c2 else None, s["dA"], s["dmA"], field)
    else:
        g, dg = s["arr"].values(s["t"], F0, SCALE)
        ref = s["y0"].astype(np.float64) + waveform_cpu.facet_reference(s["ndofs"], g, dg, s["ids"], s["c1"], s["c2"] if with_c2 else None, s["dA"], s["dmA"], field)
    return ref


def _own_ratio(kind, got, ref, T):
    if kind == "array":
        return facet_cpu.rel_inf(got, ref) / facet_cpu.ARRAY_TOL[np.dtype(T)]
    tol = TOL[np.dtype(T)]
    return max(rel_l2(got, ref) / tol["l2"], rel_max(got, ref) / tol["mx"])


def _check_facets(kind, dtype, s, with_c2, with_B, variant, gpu, oracle_c, label):
    T = s["dtype"]
    got, v1, v2 = _launch(kind, s, with_c2, with_B, variant, gpu)
    field = (s["x"], s["cB"], s["dB"], s["dmB"]) if with_B else None
    ref, mag, k = facet_cpu.reference64(s["y0"], v1, v2, s["dA"], s["dmA"], field)
    # dofs that no live facet adds to keep the bits of y0: the reserved dofs of the inactive, silent and out-of-table facets among them
    untouched = k == 0
    assert np.array_equal(_bits(got[untouched]), _bits(s["y0"][untouched])), f"{label}: a dof that nothing adds to changed"
    if s["quiet"].any():
        assert untouched[s["ndofs"] - s["reserved"]:].all() and np.unique(s["dmA"][s["quiet"]]).size > 1
    own = _own_ratio(kind, got, _own_reference(kind, s, with_c2, with_B, oracle_c), T)
    _report(KINDS[kind], dtype, f"{label}-own", own)
    assert own < 1.0, f"{label}: {own} x the tolerance of the kernel's own test"
    # per dof: (k + 3) eps (|y0| + sum |terms|); for an fp64 source kernel widened by what two fp64 evaluations of g_e may differ by
    bound = facet_cpu.dof_bound(mag, k, T)
    if kind != "terms" and T == np.float64:
        bound = bound + _evaluation_slack(kind, s, with_c2, v1)
    r = float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)))
    _report(KINDS[kind], dtype, f"{label}-dof", r)
    assert r <= 1.0, f"{label}: a dof is {r} x its bound (k + 3) eps (|y0| + sum |terms|)"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", range(1, 11))
@pytest.mark.parametrize("kind", KINDS)
def test_facet_kernels_every_degree(gpu, oracle_c, kind, P, dtype):
    """N = (P + 1)^2, 300 + 170 facets on 5000 dofs (several workgroups, the last partial): with and without the second constant, with
    and without set B, host and device scalars / stage."""
    N = (P + 1) ** 2
    s = _facet_case_inputs(kind, dtype, N, 300, 170, 5000, reserved=200)
    for with_c2 in (True, False):
        for with_B in (True, False):
            for variant in ("host", "dev"):
                _check_facets(kind, dtype, s, with_c2, with_B, variant, gpu, oracle_c, f"N{N}-c2{int(with_c2)}-B{int(with_B)}-{variant}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_facet_terms_one_dof_per_facet(gpu, oracle_c, dtype):
    """N = 1: the facet index is the entry index."""
    s = _facet_case_inputs("terms", dtype, 1, 700, 333, 400, reserved=0)
    for variant in ("host", "dev"):
        _check_facets("terms", dtype, s, True, True, variant, gpu, oracle_c, f"N1-{variant}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_facet_kernels_empty_sets(gpu, oracle_c, kind, dtype):
    """nentA = 0, nentB = 0 (a field of no rows, and no field), and both at once: no launch, y keeps its bits."""
    for nA, nB in ((0, 170), (300, 0)):
        s = _facet_case_inputs(kind, dtype, 16, nA, nB, 5000, reserved=200)
        for variant in ("host", "dev"):
            _check_facets(kind, dtype, s, True, True, variant, gpu, oracle_c, f"nA{nA}-nB{nB}-{variant}")
    s = _facet_case_inputs(kind, dtype, 16, 0, 0, 5000, reserved=0)
    for with_B in (True, False):
        got, _, _ = _launch(kind, s, True, with_B, "host", gpu)
        assert np.array_equal(_bits(got), _bits(s["y0"]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["seam_in_first_trip", "seam_in_second_trip"])
@pytest.mark.parametrize("kind", KINDS)
def test_facet_kernels_sweep(gpu, oracle_c, kind, shape, dtype):
    """41 960 facets x N = 25 = 4096 x 256 + 424 entries on 50 000 dofs (about 21 adds per dof).  First shape: set A ends inside the
    first trip and set B spans the end of the grid.  Second shape: set A alone exceeds the grid (by 174 entries: its last seven facets),
    so the seam between the sets lies in the second trip; the six of them that lie wholly in it hold an inactive facet, a time before
    the start and one past the end (of the burst; of the table), for the waveform kernel a silent row, and live facets between them."""
    b = sk.of(KINDS[kind], dtype)
    nent, N = b.sweep
    stride = b.cap * 256
    nA = 20000 if shape == "seam_in_first_trip" else nent - 10
    tail = 0 if shape == "seam_in_first_trip" else nA - stride // N
    assert (nA * N < stride) == (shape == "seam_in_first_trip") and nent * N - stride == sk.second_trip_threads(b) and tail in (0, 7)
    s = _facet_case_inputs(kind, dtype, N, nA, nent - nA, 50000, reserved=500, tail=tail)
    if tail and kind != "terms":
        second = np.arange(nA - tail + 1, nA)  # the facets of set A whose every entry lies in the second trip
        assert second[0] * N >= stride and nA * N < nent * N
        reasons = [_skip_reason(kind, s["arr"], s["t"], int(e)) for e in s["ids"][second]]
        assert set(reasons) == TAIL_REASONS[kind], reasons
        assert np.array_equal(s["quiet"][second], np.array(reasons) != "live")
    _check_facets(kind, dtype, s, True, True, "host", gpu, oracle_c, f"sweep-{shape}")


# =========================================================================================================================================
# halo_kernel
HALO_COUNTS = (0, 1, 256, 257, sk.KERNELS["halo_kernel"][3][0])
OFFSET = 1234  # the non-zero N of pack_rev and unpack_fwd


def _halo(dtype):
    import torch

    return pkg("scatterer").HipHaloKernels({"f64": torch.float64, "f32": torch.float32}[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", HALO_COUNTS)
@pytest.mark.parametrize("op", ["pack_fwd", "pack_rev"])
def test_halo_pack(gpu, op, count, dtype):
    """out[i] = in[index[i] (+ N)], indices with repeats: bitwise numpy; a count of 0 leaves the poisoned output untouched."""
    import torch

    T, k = DTYPES[dtype], _halo(dtype)
    rng = np.random.default_rng([31, count, T().itemsize])
    nsrc = max(count // 3, 7)
    off = OFFSET if op == "pack_rev" else 0
    src = rng.standard_normal(nsrc + off).astype(T)
    index = rng.integers(0, nsrc, count)
    raw, out = _guarded(shape=(count,), dtype=T)
    if op == "pack_fwd":
        k.pack_fwd(_td(src), out, k.index_tensor(index))
    else:
        k.pack_rev(_td(src), out, k.index_tensor(index), off)
    torch.cuda.synchronize()
    assert _guard_kept(raw)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(src[index + off]))
    _report("halo_kernel", dtype, f"PACK-{op}-{count}", 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", HALO_COUNTS)
def test_halo_unpack_fwd(gpu, count, dtype):
    """out[index[i] + N] = in[i], distinct indices: bitwise numpy; entries that no index names keep their bits."""
    import torch

    T, k = DTYPES[dtype], _halo(dtype)
    rng = np.random.default_rng([32, count, T().itemsize])
    ntarget = 2 * count + 9
    index = rng.permutation(ntarget)[:count]
    y0, src = rng.standard_normal(ntarget + OFFSET).astype(T), rng.standard_normal(count).astype(T)
    raw, out = _guarded(init=y0)
    k.unpack_fwd(_td(src), out, k.index_tensor(index), OFFSET)
    torch.cuda.synchronize()
    assert _guard_kept(raw)
    ref = y0.copy()
    ref[index + OFFSET] = src
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref))
    _report("halo_kernel", dtype, f"UNPACK_SET-{count}", 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", HALO_COUNTS)
def test_halo_unpack_rev(gpu, count, dtype):
    """out[index[i]] += in[i] with about 16 adds per target: per entry within (k + 3) eps (|y0| + sum |terms|) of the fp64 np.add.at;
    entries that no index names keep their bits."""
    import torch

    T, k = DTYPES[dtype], _halo(dtype)
    rng = np.random.default_rng([33, count, T().itemsize])
    ntarget = count // 16 + 5
    index = rng.integers(0, ntarget - 3, count)  # the last three entries are named by no index
    y0, src = rng.standard_normal(ntarget).astype(T), rng.standard_normal(count).astype(T)
    raw, out = _guarded(init=y0)
    k.unpack_rev(_td(src), out, k.index_tensor(index))
    torch.cuda.synchronize()
    assert _guard_kept(raw)
    got = out.cpu().numpy()
    ref, mag, n = y0.astype(np.float64), np.abs(y0.astype(np.float64)), np.zeros(ntarget, dtype=np.int64)
    np.add.at(ref, index, src.astype(np.float64))
    np.add.at(mag, index, np.abs(src.astype(np.float64)))
    np.add.at(n, index, 1)
    assert np.array_equal(_bits(got[n == 0]), _bits(y0[n == 0])) and (n == 0).sum() >= 3
    r = float(np.max(np.abs(got.astype(np.float64) - ref) / facet_cpu.dof_bound(mag, n, T)))
    _report("halo_kernel", dtype, f"UNPACK_ADD-{count}", r)
    assert r <= 1.0
    if count > 1000:
        assert n.max() > 16


def test_halo_pack_rev_beyond_2_31_elements(gpu):
    """fp32 pack_rev whose source has 2^31 + 1024 elements (8.6 GB): only the last 2048 are filled and 1000 indices, with N = 2^31 - 1024,
    point into them on either side of element 2^31: ``index + offset`` stays 64-bit."""
    import torch

    k = _halo("f32")
    rng = np.random.default_rng(34)
    total, tail = 2**31 + 1024, 2048
    N = total - tail
    src = torch.empty(total, dtype=torch.float32, device="cuda")
    values = rng.standard_normal(tail).astype(np.float32)
    src[N:] = _td(values)
    index = rng.integers(0, tail, 1000)
    assert (index + N < 2**31).any() and (index + N >= 2**31).any()
    raw, out = _guarded(shape=(1000,), dtype=np.float32)
    k.pack_rev(src, out, k.index_tensor(index), N)
    torch.cuda.synchronize()
    assert _guard_kept(raw)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(values[index]))
    del src
    torch.cuda.empty_cache()
