"""Sampled source waveforms on the host (sources.SampledWaveform, ``waveform=`` of SourceArray / PointSources,
receivers.time_reversed_waveform): the order of the interpolant, exactness and edges, a sampled analytic source against the analytic
one, validation, the C ABI of include/fus_gpu_waveform.h and the register pins of csrc/source_wave.hpp."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import waveform_cpu
from conftest import ROOT, pkg

F0 = 0.5e6
T0 = 1.0 / F0
ENTRY_POINTS = [f"fus_{k}_{s}" for k in ("facet_source_wave", "facet_source_wave_dev", "point_source_wave") for s in ("f64", "f32")]


# ---- 1. the order of the interpolant ---------------------------------------------------------------------------------------------------
def test_interpolant_is_fourth_order_in_the_value_and_third_in_the_derivative():
    """A Gaussian-modulated cosine on [0, 8 T], 16 / 32 / 64 / 128 samples per period, stencil derivative, 20 001 evaluation points.
    numpy gives value errors 9.0e-5, 4.8e-6, 2.8e-7, 1.75e-8 (factors 19, 16.8, 16.2) and derivative errors over w0 of 9.4e-4, 7.4e-5,
    8.9e-6, 1.1e-6 (factors 12.7, 8.3, 8.1): each halving must divide the value error by at least 12 and the derivative's by 6."""
    src = pkg("sources")
    w0 = 2 * np.pi * F0
    te = np.linspace(0.0, 8 * T0, 20001)
    ge, dge = waveform_cpu.gaussian_pulse(te, F0, 4 * T0)
    ev, ed = [], []
    for N in (16, 32, 64, 128):
        dt = T0 / N
        wf = src.SampledWaveform(waveform_cpu.gaussian_pulse(np.arange(8 * N + 1) * dt, F0, 4 * T0)[0], dt)
        w, dw = wf.values(te)
        ev.append(np.abs(w - ge).max())
        ed.append(np.abs(dw - dge).max() / w0)
    print("value errors", ev, "derivative errors / w0", ed)
    assert ev[0] < 2e-4 and ed[0] < 2e-3
    for i in range(3):
        assert ev[i] / ev[i + 1] >= 12.0, (i, ev)
        assert ed[i] / ed[i + 1] >= 6.0, (i, ed)


def test_stencil_derivative_is_exact_for_quartics_up_to_the_ends():
    """The five-point stencils, central and one-sided, differentiate a polynomial of degree 4 exactly: no zero padding at the ends."""
    src = pkg("sources")
    t = np.arange(9) * 0.25
    f = 1.0 + t - 2 * t**2 + 0.5 * t**3 - 0.25 * t**4
    d = 1.0 - 4 * t + 1.5 * t**2 - t**3
    assert np.max(np.abs(src.stencil_derivative(f, 0.25) - d)) < 1e-12 * np.max(np.abs(d))
    assert np.allclose(src.stencil_derivative(np.array([1.0, 3.0]), 0.5), [4.0, 4.0])  # Nt = 2: the difference quotient
    assert np.allclose(src.stencil_derivative(np.array([0.0, 1.0, 4.0]), 1.0), [0.0, 2.0, 4.0])  # Nt = 3: second order


# ---- 2. exactness and edges --------------------------------------------------------------------------------------------------------------
def test_nodes_are_exact_and_the_outside_is_zero():
    src = pkg("sources")
    rng = np.random.default_rng(0)
    Nt, dt, t0 = 37, 2.0**-22, 3 * 2.0**-22  # a power of two: node times and (s - t0) / dt are exact
    w, d = rng.standard_normal((3, Nt)), rng.standard_normal((3, Nt)) / dt
    wf = src.SampledWaveform(w, dt, t0=t0, derivative=d)
    nodes = t0 + np.arange(Nt) * dt
    for r in range(3):
        got, dgot = wf.values(nodes, r)
        assert np.array_equal(got.view(np.int64), w[r].view(np.int64))  # 0 ulp, the last node (k = Nt - 2, th = 1) included
        assert np.array_equal(dgot.view(np.int64), d[r].view(np.int64))
    below, above = np.nextafter(t0, -np.inf), np.nextafter(nodes[-1], np.inf)
    for s in (below, above, -1.0, 1.0, np.nan, np.inf, -np.inf):
        got, dgot = wf.values(s, 1)
        assert got == 0.0 and dgot == 0.0, s
    inside, _ = wf.values(np.nextafter(nodes[-1], -np.inf), 2)
    assert abs(inside - w[2, -1]) < 1e-9 * abs(w[2, -1])  # just inside the last interval: k = Nt - 2, th just below 1
    assert wf.t_end == nodes[-1]
    # rows outside [0, R) are silent, and s and rows broadcast
    got, _ = wf.values(nodes[5], [-1, 0, 3, 2])
    assert got.tolist() == [0.0, w[0, 5], 0.0, w[2, 5]]
    # C1: value and derivative are continuous across a node
    eps = dt * 1e-7
    (a, da), (b, db) = wf.values(nodes[9] - eps, 0), wf.values(nodes[9] + eps, 0)
    assert abs(a - b) < 1e-5 * np.abs(w).max() and abs(da - db) < 1e-5 * np.abs(d).max()
    # the table of the kernels: value and derivative interleaved
    tab = wf.table()
    assert tab.shape == (3, Nt, 2) and tab.flags.c_contiguous and np.array_equal(tab[..., 0], w) and np.array_equal(tab[..., 1], d)
    assert np.array_equal(wf.table([2, 0])[1, :, 0], w[0])


def test_two_samples_are_a_table():
    src = pkg("sources")
    wf = src.SampledWaveform([2.0, 4.0], 0.5, t0=1.0)
    assert wf.n_rows == 1 and wf.n_samples == 2 and np.allclose(wf.derivative, 4.0)
    w, dw = wf.values([0.99, 1.0, 1.25, 1.5, 1.51])
    assert np.allclose(w, [0.0, 2.0, 3.0, 4.0, 0.0]) and np.allclose(dw, [0.0, 4.0, 4.0, 4.0, 0.0])  # a line is reproduced


def test_from_pressure():
    """w = (dp/dt) / (p0 w0): the surface pressure p0 sin(w0 t) gives the solvers' cosine."""
    src = pkg("sources")
    dt = T0 / 64
    t = np.arange(4 * 64 + 1) * dt
    wf = src.SampledWaveform.from_pressure(6e4 * np.sin(2 * np.pi * F0 * t), dt, 6e4, F0, t0=1e-6)
    assert wf.t0 == 1e-6 and wf.n_rows == 1
    # the stencils' truncation terms: h^4 f^(5) / 30 (central), h^4 f^(5) / 20 (second sample), h^4 f^(5) / 5 (end sample); for a
    # sine that is (w0 h)^4 / 30 and / 5 of the amplitude, 3.1e-6 and 1.86e-5 at 64 samples per period (the next order adds 5 %)
    err, x4 = np.abs(wf.samples[0] - np.cos(2 * np.pi * F0 * t)), (2 * np.pi / 64) ** 4
    assert err.max() < 1.1 * x4 / 5 and err[2:-2].max() < 1.1 * x4 / 30


# ---- 3. a sampled analytic source is the analytic source ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["linear", "westervelt"])
def test_sampled_analytic_source_is_the_analytic_source(which):
    """The analytic waveform sampled at half the solver step with its analytic derivative: every stage time of 40 steps is a node, so
    ``values`` equals ``_waveform`` to 1e-14 of the largest value, g and dg, at the linear and at the Westervelt source scale."""
    src = pkg("sources")
    f0, scale = (F0, 6e4 * 2 * np.pi * F0 / 1500.0) if which == "linear" else (1.1e6, 2 * 5.7e5 * 2 * np.pi * 1.1e6 / 1480.0)
    dt = 1.0 / f0 / 24
    amp, phase, delay = np.array([1.0, 0.4, 1.3]), np.array([0.0, 0.9, -2.0]), np.array([0.0, 3.0, 7.0]) * 0.5 * dt
    ana = src.SourceArray([0, 1, 2], amplitude=amp, phase=phase, delay=delay)
    wf = waveform_cpu.analytic_table(ana, f0, 0.5 * dt, 2 * 40 + 2)  # one sample past the last stage time, whose x may round above 80
    sam = src.SourceArray([0, 1, 2], amplitude=amp, delay=delay, waveform=wf)
    assert sam.waveform_of_element.tolist() == [0, 1, 2]
    times = [n * dt + c * dt for n in range(40) for c in (0.0, 0.5, 0.5, 1.0)]
    ref = np.array([ana.values(t, f0, scale) for t in times])
    got = np.array([sam.values(t, f0, scale) for t in times])
    for k, name in enumerate(("g", "dg")):
        big = np.abs(ref[:, k]).max()
        assert big > 0 and np.abs(got[:, k] - ref[:, k]).max() <= 1e-14 * big, name


def test_point_sources_share_the_rules():
    src = pkg("sources")
    wf = src.SampledWaveform([[0.0, 1.0, 0.0], [0.0, -2.0, 0.0]], 1.0)
    ps = src.PointSources(np.zeros((2, 3)), amplitude=[2.0, 3.0], delay=[0.0, 0.5], waveform=wf)
    assert ps.waveform_of_point.tolist() == [0, 1]
    g, dg = ps.values(1.0, F0)
    assert g[0] == 2.0 and g[1] == 3.0 * wf.values(0.5, 1)[0] and dg[1] == 3.0 * wf.values(0.5, 1)[1]
    one = src.PointSources(np.zeros((2, 3)), waveform=src.SampledWaveform([0.0, 1.0], 1.0), waveform_of_point=[0, -1])
    assert one.values(1.0, F0)[0].tolist() == [1.0, 0.0]


# ---- 4. validation -----------------------------------------------------------------------------------------------------------------------
def test_validation_errors():
    src = pkg("sources")
    W = src.SampledWaveform
    ok = W(np.zeros((3, 4)), 1.0)
    with pytest.raises(ValueError, match="Nt >= 2"):
        W([1.0], 1.0)
    with pytest.raises(ValueError, match=r"\[R, Nt\]"):
        W(np.zeros((2, 3, 4)), 1.0)
    with pytest.raises(ValueError, match=r"\[R, Nt\]"):
        W(np.zeros((0, 4)), 1.0)
    with pytest.raises(ValueError, match="finite"):
        W([0.0, np.nan, 1.0], 1.0)
    with pytest.raises(ValueError, match="finite"):
        W([0.0, np.inf], 1.0)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="dt"):
            W([0.0, 1.0], bad)
    with pytest.raises(ValueError, match="t0"):
        W([0.0, 1.0], 1.0, t0=np.nan)
    with pytest.raises(ValueError, match="derivative"):
        W(np.zeros((2, 4)), 1.0, derivative=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="derivative"):
        W([0.0, 1.0], 1.0, derivative=[0.0, np.nan])
    # phase / duration belong to the analytic form
    with pytest.raises(ValueError, match="phase and duration"):
        src.SourceArray([0, 1, 2], waveform=ok, phase=[0.0, 0.1, 0.0])
    with pytest.raises(ValueError, match="phase and duration"):
        src.SourceArray([0, 1, 2], waveform=ok, duration=1e-5)
    with pytest.raises(ValueError, match="phase and duration"):
        src.PointSources(np.zeros((3, 3)), waveform=ok, phase=0.5)
    with pytest.raises(ValueError, match="SampledWaveform"):
        src.SourceArray([0], waveform=np.zeros((1, 4)))
    # the row map
    with pytest.raises(ValueError, match="neither 1 nor 2"):
        src.SourceArray([0, 1], waveform=ok)
    with pytest.raises(ValueError, match="neither 1 nor 4"):
        src.PointSources(np.zeros((4, 3)), waveform=ok)
    with pytest.raises(ValueError, match=r"\[-1, 3\)"):
        src.SourceArray([0, 1], waveform=ok, waveform_of_element=[0, 3])
    with pytest.raises(ValueError, match=r"\[-1, 3\)"):
        src.SourceArray([0, 1], waveform=ok, waveform_of_element=[-2, 0])
    with pytest.raises(ValueError, match="one integer row"):
        src.SourceArray([0, 1], waveform=ok, waveform_of_element=[0, 1, 2], n_elements=2)
    with pytest.raises(ValueError, match="one integer row"):
        src.SourceArray([0, 1], waveform=ok, waveform_of_element=[0.0, 1.0])
    with pytest.raises(ValueError, match="needs waveform"):
        src.SourceArray([0, 1], waveform_of_element=[0, 1])
    with pytest.raises(ValueError, match="needs waveform"):
        src.PointSources(np.zeros((2, 3)), waveform_of_point=[0, 1])
    # what is allowed: R == 1, R == E, a map with silent elements; the length of the map gives E
    assert src.SourceArray([0, 1], waveform=W([0.0, 1.0], 1.0)).waveform_of_element.tolist() == [0, 0]
    assert src.SourceArray([0, 1, 2], waveform=ok).waveform_of_element.tolist() == [0, 1, 2]
    assert src.SourceArray(lambda c: np.zeros(len(c), int), waveform=ok, waveform_of_element=[2, -1, 0, 0]).n_elements == 4
    # without waveform= nothing changes
    a = src.SourceArray([0, 1], phase=[0.1, 0.2], duration=1e-4)
    assert a.waveform is None and a.waveform_of_element is None and src.PointSources(np.zeros((1, 3))).waveform is None


# ---- 5. the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_declared_bound_and_exported():
    lib_mod = pkg("_lib")
    path = os.path.join(ROOT, "include", "fus_gpu_waveform.h")
    assert lib_mod.LATER_HEADER_PATHS[-1] == path
    hdr = open(path).read()
    lib = lib_mod.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in lib_mod.LATER, name
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes == lib_mod.LATER[name][1]
    i64, dbl, ptr = C.c_int64, C.c_double, C.c_void_p
    assert lib_mod.LATER["fus_point_source_wave_f32"][1] == [ptr, ptr, i64, ptr, i64, ptr, C.c_int, ptr, ptr, ptr, ptr, i64, i64, dbl, dbl,
                                                             ptr, ptr]
    assert lib_mod.LATER["fus_facet_source_wave_dev_f64"][1] == [ptr] * 6 + [i64] + [ptr] * 3 + [i64, ptr, i64, i64, dbl, dbl] + [ptr] * 4 + [
        i64, C.c_int, ptr, ptr]


def test_abi_argument_checks_precede_device_work():
    lib = pkg("_lib").load()
    z, one = C.c_void_p(0), C.c_void_p(256)  # ``one``: non-null, 16-byte aligned, never dereferenced: validation fails first
    stage = (C.c_double * 6)(0.0, 2 * np.pi * F0, 1.0, F0, 4.0, 0.0)
    sp = C.cast(stage, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    for suf in ("f64", "f32"):
        for dev in ("", "dev_"):
            fn = getattr(lib, f"fus_facet_source_wave_{dev}{suf}")

            def call(y=one, c1=one, c2=z, dA=one, dmA=one, eid=one, nA=1, a=one, tau=one, row=one, E=1, tab=one, R=1, Nt=2, t0=0.0, dt=1.0,
                     xB=z, cB=z, dB=z, dmB=z, nB=0, N=9, st=sp):
                return fn(y, c1, c2, dA, dmA, eid, nA, a, tau, row, E, tab, R, Nt, t0, dt, xB, cB, dB, dmB, nB, N, st, z)

            assert call(y=z, c1=z, dA=z, dmA=z, eid=z, nA=0, a=z, tau=z, row=z, E=0, tab=z, R=0, Nt=0, st=z) == 0  # zero-size: no-op
            assert call(nA=-1) == -1 and call(nB=-1) == -1 and call(E=-1) == -1 and call(N=0) == -1
            assert call(E=0) == -1
            assert call(y=z) == -1 and call(st=z) == -1
            for k in ("c1", "dA", "dmA", "eid", "a", "tau", "row", "tab"):
                assert call(**{k: z}) == -1, k
            assert call(R=0) == -1 and call(R=-3) == -1 and call(Nt=1) == -1 and call(Nt=0) == -1
            for bad in (0.0, -1.0, nan, inf):
                assert call(dt=bad) == -1, bad
            assert call(t0=nan) == -1 and call(t0=inf) == -1
            assert call(tab=C.c_void_p(264)) == -1  # the table's intervals are read with 16-byte loads
            assert call(a=C.c_void_p(260)) == -1 and call(row=C.c_void_p(258)) == -1
            assert call(nA=0, nB=2) == -1  # set B with null pointers
            assert call(nA=0, E=0, nB=2, xB=one, cB=one, dB=one, dmB=z) == -1
        fn = getattr(lib, f"fus_point_source_wave_{suf}")

        def pcall(y=one, cells=one, m=1, dm=one, nc=1, w=one, P=2, a=one, tau=one, row=one, tab=one, R=1, Nt=2, t0=0.0, dt=1.0, st=sp):
            return fn(y, cells, m, dm, nc, w, P, a, tau, row, tab, R, Nt, t0, dt, st, z)

        assert pcall(y=z, cells=z, m=0, dm=z, nc=0, w=z, a=z, tau=z, row=z, tab=z, R=0, Nt=0, st=z) == 0  # no points: no-op
        assert pcall(m=-1) == -1 and pcall(nc=-1) == -1
        assert pcall(P=0) != 0 and pcall(P=11) != 0 and pcall(P=0) == pcall(P=11) != -1  # FUS_ERR_UNSUPPORTED_DEGREE
        for k in ("y", "cells", "dm", "w", "a", "tau", "row", "tab", "st"):
            assert pcall(**{k: z}) == -1, k
        assert pcall(R=0) == -1 and pcall(Nt=1) == -1
        for bad in (0.0, -1.0, nan, inf):
            assert pcall(dt=bad) == -1, bad
        assert pcall(t0=nan) == -1 and pcall(tab=C.c_void_p(264)) == -1 and pcall(tau=C.c_void_p(260)) == -1


# ---- 6. resource pins ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_wave_kernels_resource_pin():
    """The pin of the kernels they stand beside (csrc/source_array.hpp: they run next to a launch that holds the CUs): at most 64
    VGPRs, no AGPRs, no scratch, no LDS, 8 waves per SIMD, both types, every degree of the point kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    table = ru.parse(ru.cached_remarks())
    names = [rf"facet_source_wave_kernel<{T}>" for T in ("double", "float")]
    names += [rf"point_source_wave_kernel<{T}, {P}>" for T in ("double", "float") for P in range(1, 11)]
    for name in names:
        hits = [(k, v) for k, v in table.items() if re.search(name, k)]
        assert len(hits) == 1, (name, hits)
        d = hits[0][1]
        assert d["scratch"] == 0 and d["agpr"] == 0 and d["vgpr"] <= 64 and d["occupancy"] >= 8 and d["lds"] == 0, (name, d)


# ---- 7. time_reversed_waveform on the host -------------------------------------------------------------------------------------------------
def test_time_reversed_waveform():
    src, rx = pkg("sources"), pkg("receivers")
    rng = np.random.default_rng(3)
    nrec, E, dt = 41, 5, 1e-7
    S = rng.standard_normal((nrec, E)) * np.array([1.0, 0.5, 0.0, 2.0, 1.0])
    S[:, 4] = np.nan  # an element without facets: the area average is NaN
    ids = np.array([0, 1, 2, 3, 4, 4])
    arr = rx.time_reversed_waveform(S, dt, element_of_facet=ids)
    wf = arr.waveform
    assert isinstance(arr, src.SourceArray) and arr.n_elements == E and wf.n_rows == E and wf.n_samples == nrec
    assert wf.dt == dt and wf.t0 == 0.0
    assert arr.waveform_of_element.tolist() == [0, 1, -1, 3, -1]  # silent: heard nothing, or NaN
    assert np.all(arr.amplitude == 1.0) and np.all(arr.delay == 0.0)
    for e in (0, 1, 3):  # "uniform": every row by its own largest value; reversed in time
        assert np.allclose(wf.samples[e], S[::-1, e] / np.abs(S[:, e]).max(), rtol=1e-15, atol=0)
        assert np.abs(wf.samples[e]).max() == 1.0
    assert not np.any(wf.samples[2]) and not np.any(wf.samples[4])
    # what element e emits at time s is what it heard at T_rec - s
    g, _ = arr.values(7 * dt, F0, 2.0)
    assert np.allclose(g[[0, 1, 3]], 2.0 * S[nrec - 1 - 7, [0, 1, 3]] / np.abs(S[:, [0, 1, 3]]).max(axis=0)) and g[2] == 0.0 and g[4] == 0.0
    rec = rx.time_reversed_waveform(S, dt, element_of_facet=ids, amplitude="recorded").waveform
    big = np.abs(S[:, [0, 1, 3]]).max()
    for e in (0, 1, 3):  # "recorded": every row by the largest over all elements
        assert np.allclose(rec.samples[e], S[::-1, e] / big, rtol=1e-15, atol=0)
    assert np.abs(rec.samples).max() == 1.0 and np.abs(rec.samples[1]).max() < 1.0
    # the taper: a cosine ramp over a fraction of the window at each end
    tap = rx.time_reversed_waveform(S, dt, element_of_facet=ids, taper=0.25).waveform
    nt = 10
    ramp = 0.5 * (1.0 - np.cos(np.pi * np.arange(nt) / nt))
    win = np.ones(nrec)
    win[:nt], win[-nt:] = ramp, ramp[::-1]
    assert np.allclose(tap.samples[0], wf.samples[0] * win, rtol=1e-15, atol=0) and tap.samples[0, 0] == 0.0 and tap.samples[0, -1] == 0.0
    assert np.array_equal(tap.samples[:, nt:-nt], wf.samples[:, nt:-nt])
    # errors
    with pytest.raises(ValueError, match="no element received anything"):
        rx.time_reversed_waveform(np.zeros((5, 3)), dt, element_of_facet=[0, 1, 2])
    with pytest.raises(ValueError, match="no element received anything"):
        rx.time_reversed_waveform(np.full((5, 2), np.nan), dt, element_of_facet=[0, 1])
    with pytest.raises(ValueError, match="element_of_facet"):
        rx.time_reversed_waveform(S, dt)
    with pytest.raises(ValueError, match="amplitude"):
        rx.time_reversed_waveform(S, dt, element_of_facet=ids, amplitude="conjugate")
    with pytest.raises(ValueError, match="taper"):
        rx.time_reversed_waveform(S, dt, element_of_facet=ids, taper=0.6)
    with pytest.raises(ValueError, match="two records"):
        rx.time_reversed_waveform(S[:1], dt, element_of_facet=ids)
