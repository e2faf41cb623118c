"""Phased-array sources on the host (sources.py) and the C ABI's argument checks of fus_facet_source_array_* (no device
work): the one-element array is today's source, the burst envelope, element assignment by centroid, the focus / steer
helpers, validation, and the register pin of the new kernel."""
import ctypes as C
import os
import re
import shutil
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, pkg

F0_LIN, F0_NL = 0.5e6, 1.1e6


def _lin_stub(f0=F0_LIN, p0=60000.0, c0=1500.0):
    return types.SimpleNamespace(f0=f0, p0=p0, c0=c0, w0=2.0 * np.pi * f0)


def _times(f0, n=1000):
    """n times over 12 periods, with the ramp edges (0, alpha T) and points just either side of them."""
    T = 1.0 / f0
    t = np.linspace(0.0, 12 * T, n - 6)
    return np.concatenate([t, [4 * T, np.nextafter(4 * T, 0), np.nextafter(4 * T, 1), 1e-300, 0.5 * T, 3.999 * T]])


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_one_element_array_is_todays_linear_source():
    ls, src = pkg("linear_solver"), pkg("sources")
    stub = _lin_stub()
    arr = src.SourceArray(np.zeros(4, np.int64))
    A = stub.p0 * stub.w0 / stub.c0
    ts = _times(stub.f0)
    ref = np.array([ls.LinearSpectral3D.source_value(stub, t) for t in ts])
    got = np.array([arr.values(t, stub.f0, A)[0][0] for t in ts])
    assert np.max(np.abs(ref)) > 0 and _rel(got, ref) <= 1e-15
    assert got[0] == 0.0 and ref[0] == 0.0


def test_one_element_array_is_todays_westervelt_source():
    nl, src = pkg("nonlinear_solver"), pkg("sources")
    stub = types.SimpleNamespace(f0=F0_NL, p0=1000.0 * 1480.0 * 0.38557513826589934, c0=1480.0, w0=2 * np.pi * F0_NL)
    arr = src.SourceArray([0], n_elements=1)
    A = 2.0 * stub.p0 * stub.w0 / stub.c0
    ts = _times(stub.f0)
    ref = np.array([nl.WesterveltSpectral3D.source_values(stub, t) for t in ts])
    got = np.array([[v[0] for v in arr.values(t, stub.f0, A)] for t in ts])
    assert _rel(got[:, 0], ref[:, 0]) <= 1e-15 and _rel(got[:, 1], ref[:, 1]) <= 1e-15


@pytest.mark.parametrize("duration", [None, 9.5e-6], ids=["cw", "burst"])
def test_derivative_matches_central_difference(duration):
    src = pkg("sources")
    f0, A = F0_LIN, 3.0
    arr = src.SourceArray([0, 1, 2], amplitude=[1.0, 0.5, 2.0], phase=[0.0, 1.0, -2.5], delay=[0.0, 1.3e-6, 3.1e-6], duration=duration)
    h = 1e-12
    for t in np.linspace(1e-7, 14e-6, 157):
        g1, _ = arr.values(t + h, f0, A)
        g0, _ = arr.values(t - h, f0, A)
        _, dg = arr.values(t, f0, A)
        scale = A * 2 * np.pi * f0 * 2.0
        assert np.max(np.abs((g1 - g0) / (2 * h) - dg)) <= 2e-6 * scale, t


def test_burst_envelope_edges():
    src = pkg("sources")
    f0, alpha = F0_LIN, 4.0
    T = 1.0 / f0
    D = 10 * T
    tau = 1.5 * T
    arr = src.SourceArray([0], delay=tau, duration=D)
    env = lambda t: arr.values(t, f0, 1.0)[0][0] / np.cos(2 * np.pi * f0 * (t - tau))  # noqa: E731
    # before the delay, at the start and after the end: exactly zero
    for t in (0.0, 0.5 * tau, tau, tau + D, tau + D + 0.3 * T, tau + 20 * T):
        assert arr.values(t, f0, 1.0)[0][0] == 0.0 and arr.values(t, f0, 1.0)[1][0] == 0.0, t
    # plateau between the ramps: the carrier alone
    for t in tau + np.array([alpha * T + 0.1 * T, 5.0 * T, D - alpha * T - 0.13 * T]):
        assert abs(env(t) - 1.0) < 1e-12
    # the ramp down mirrors the ramp up
    for x in (0.3 * T, 1.7 * T, 3.2 * T):
        up = 0.5 * (1 - np.cos(np.pi * f0 * x / alpha))
        assert abs(env(tau + x) - up) < 1e-12 and abs(env(tau + D - x) - up) < 1e-12
    with pytest.raises(ValueError, match="shorter"):
        src.SourceArray([0], duration=7 * T).check_duration(f0)
    src.SourceArray([0], duration=8 * T).check_duration(f0)
    blk = arr.stage_scalars(2e-6, f0, 5.0)
    assert blk.dtype == np.float64 and blk.tolist() == [2e-6, 2 * np.pi * f0, 5.0, f0, 4.0, D]
    assert src.SourceArray([0]).stage_scalars(0.0, f0, 1.0)[5] == 0.0


def _array_mesh(P=2, cells=(3, 4, 2), L=0.01):
    boxmesh, ad = pkg("boxmesh"), pkg("dolfinx_adaptor")
    box = boxmesh.BoxMesh(P, cells, length=L, perturb=0.1, seed=4)
    rng = np.random.default_rng(5)
    cperm, vperm = rng.permutation(box.ncells), rng.permutation(box.x_g.shape[0])
    vinv = np.empty_like(vperm)
    vinv[vperm] = np.arange(vperm.size)
    tags = {1: box.boundary_facets([2]), 2: box.boundary_facets([3])}
    inv = np.empty_like(cperm)
    inv[cperm] = np.arange(cperm.size)
    tags = {k: np.stack([inv[v[:, 0]], v[:, 1]], axis=1) for k, v in tags.items()}
    return box, ad.ArrayMesh(P, box.dofmap[cperm], vinv[box.x_dofs[cperm]], box.x_g[vperm], facet_tags=tags)


def test_facet_centroids_and_assignment_on_box_and_array_mesh():
    src = pkg("sources")
    boxmesh = pkg("boxmesh")
    L = 0.01
    box = boxmesh.BoxMesh(3, (2, 4, 3), length=L)
    bd = box.boundary_facets([2])
    cen = src.facet_centroids(box, bd)
    assert cen.shape == (12, 3) and np.all(cen[:, 0] == 0.0)
    assert np.allclose(sorted(set(np.round(cen[:, 1] / L * 8, 9))), [1, 3, 5, 7])
    assert np.allclose(sorted(set(np.round(cen[:, 2] / L * 6, 9))), [1, 3, 5])
    # x = L face
    assert np.allclose(src.facet_centroids(box, box.boundary_facets([3]))[:, 0], L)
    ids_fn = src.grid_elements(2, 3, (0.0, L), (0.0, L))
    ids = src.SourceArray(ids_fn, n_elements=6).assign(box, bd)
    assert ids.dtype == np.int32 and sorted(np.bincount(ids).tolist()) == [2] * 6
    c = src.element_centres(box, bd, ids)
    assert np.allclose(c, src.grid_centres(2, 3, 0.0, (0.0, L), (0.0, L)))
    # a cell-permuted ArrayMesh (perturbed vertices): the same facets get the same elements by position
    box2, am = _array_mesh()
    b1, b2 = box2.boundary_facets([2]), am.boundary_facets([am.source_tag])
    c1, c2 = src.facet_centroids(box2, b1), src.facet_centroids(am, b2)
    o1, o2 = np.lexsort(c1.T), np.lexsort(c2.T)
    assert np.allclose(c1[o1], c2[o2], atol=1e-15)
    fn = src.grid_elements(3, 2, (0.0, 0.01), (0.0, 0.01))
    arr = src.SourceArray(fn, n_elements=6)
    assert np.array_equal(arr.assign(box2, b1)[o1], arr.assign(am, b2)[o2])


def test_focus_and_steer_helpers():
    src = pkg("sources")
    rng = np.random.default_rng(3)
    centres = np.concatenate([np.zeros((9, 1)), rng.random((9, 2)) * 0.02], axis=1)
    focus, c, f = np.array([0.03, 0.01, 0.012]), 1500.0, 0.5e6
    tau = src.focus_delays(centres, focus, c)
    d = np.linalg.norm(centres - focus, axis=1)
    assert tau.min() == 0.0 and tau[np.argmax(d)] == 0.0 and np.all(tau >= 0)
    arrival = tau + d / c
    assert np.ptp(arrival) < 1e-18
    phi = src.focus_phases(centres, focus, c, f)
    assert np.all(phi > -np.pi) and np.all(phi <= np.pi)
    assert np.allclose(np.exp(1j * phi), np.exp(-2j * np.pi * f * tau))
    # steering: a plane wave along k leaves every element's wavefront on one plane normal to k
    k = np.array([1.0, np.tan(0.3), 0.0])
    st = src.steer_delays(centres, k, c)
    kh = k / np.linalg.norm(k)
    plane = c * st - centres @ kh
    assert st.min() == 0.0 and np.ptp(plane) < 1e-15
    assert np.allclose(src.steer_delays(centres, [1, 0, 0], c), 0.0)  # broadside: centres on x = 0
    with pytest.raises(ValueError):
        src.steer_delays(centres, [0, 0, 0], c)
    # mirrored layout, mirrored steering: mirrored delays
    cm = centres * [1, -1, 1]
    assert np.allclose(src.steer_delays(cm, k * [1, -1, 1], c), st)


def test_validation_errors():
    src = pkg("sources")
    boxmesh = pkg("boxmesh")
    box = boxmesh.BoxMesh(2, (2, 2, 2), length=0.01)
    bd = box.boundary_facets([2])
    with pytest.raises(ValueError, match="one value per element"):
        src.SourceArray([0, 1, 1, 0], amplitude=[1, 2, 3], n_elements=2)
    with pytest.raises(ValueError, match="different lengths"):
        src.SourceArray([0, 1], amplitude=[1, 2], phase=[0, 1, 2])
    with pytest.raises(ValueError, match="n_elements"):
        src.SourceArray([0], n_elements=0)
    with pytest.raises(ValueError, match="duration"):
        src.SourceArray([0], duration=-1.0)
    with pytest.raises(ValueError, match="finite"):
        src.SourceArray([0], delay=[np.nan])
    with pytest.raises(ValueError, match="int array"):
        src.SourceArray(np.zeros(4))
    with pytest.raises(ValueError, match=r"ids for 4 source facets"):
        src.SourceArray([0, 0, 0]).assign(box, bd)
    with pytest.raises(ValueError, match=r"\[-1, 2\)"):
        src.SourceArray([0, 1, 2, 0], n_elements=2).assign(box, bd)
    with pytest.raises(ValueError, match=r"\[-1, 2\)"):
        src.SourceArray([0, -2, 1, 0]).assign(box, bd)
    with pytest.raises(ValueError, match="integer"):
        src.SourceArray(lambda c: c[:, 1]).assign(box, bd)
    assert src.SourceArray([0, -1, 1, -1]).assign(box, bd).tolist() == [0, -1, 1, -1]
    assert src.SourceArray([0, 3, 1, 2]).n_elements == 4
    assert src.SourceArray(lambda c: np.zeros(len(c), int), delay=[0.0, 1e-6]).n_elements == 2


def test_abi_argument_checks_precede_device_work():
    lib = pkg("_lib").load()
    z = C.c_void_p(0)
    one = C.c_void_p(256)  # non-null, never dereferenced: validation fails first
    stage = (C.c_double * 6)(0.0, 2 * np.pi * 5e5, 1.0, 5e5, 4.0, 0.0)
    sp = C.cast(stage, C.c_void_p)
    for suf in ("f64", "f32"):
        for dev in ("", "dev_"):
            fn = getattr(lib, f"fus_facet_source_array_{dev}{suf}")

            def call(y=one, c1=one, c2=z, dA=one, dmA=one, eid=one, nA=1, a=one, ph=one, tau=one, E=1, xB=z, cB=z, dB=z, dmB=z, nB=0,
                     N=9, st=sp):
                return fn(y, c1, c2, dA, dmA, eid, nA, a, ph, tau, E, xB, cB, dB, dmB, nB, N, st, z)

            assert call(y=z, c1=z, dA=z, dmA=z, eid=z, nA=0, a=z, ph=z, tau=z, E=0, st=z) == 0  # zero-size: no-op
            assert call(nA=-1) == -1 and call(nB=-1) == -1 and call(E=-1) == -1 and call(N=0) == -1
            assert call(E=0) == -1  # an array needs an element
            assert call(y=z) == -1 and call(st=z) == -1
            for k in ("c1", "dA", "dmA", "eid", "a", "ph", "tau"):
                assert call(**{k: z}) == -1, k
            assert call(nA=0, nB=2) == -1  # set B with null pointers
            assert call(nA=0, E=0, nB=2, xB=one, cB=one, dB=one, dmB=z) == -1
            assert call(a=C.c_void_p(260)) == -1  # fp64 table not 8-byte aligned
            if not dev:  # the plain variant checks the host block
                for bad in ((3, 0.0), (4, 0.0), (5, -1.0), (3, float("nan"))):
                    st2 = (C.c_double * 6)(*stage)
                    st2[bad[0]] = bad[1]
                    assert call(st=C.cast(st2, C.c_void_p)) == -1, bad


def test_declared_and_bound():
    lib_mod = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "fus_gpu.h")).read()
    for name in ("fus_facet_source_array_f64", "fus_facet_source_array_f32", "fus_facet_source_array_dev_f64", "fus_facet_source_array_dev_f32"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in lib_mod.SIGNATURES
    assert "FacetSourceArray" in open(os.path.join(ROOT, "include", "fus_gpu.hpp")).read()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_source_array_kernel_resource_pin():
    """The launch runs next to a chip-filling stiffness launch (a boundary term of the overlapped schedule): no scratch, at most
    64 VGPRs, at least 8 waves per SIMD, for both types."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    table = ru.parse(ru.cached_remarks())
    for T in ("double", "float"):
        hits = [(k, v) for k, v in table.items() if re.search(rf"facet_source_array_kernel<{T}>", k)]
        assert len(hits) == 1, hits
        d = hits[0][1]
        assert d["scratch"] == 0 and d["agpr"] == 0 and d["vgpr"] <= 64 and d["occupancy"] >= 8, (T, d)
