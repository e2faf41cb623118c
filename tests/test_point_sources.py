"""Point sources on the host (sources.PointSources, sources.claim_points), the C ABI's argument checks of fus_point_source_* (no device
work), the header / binding, and the resource pin of the kernel."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import point_source_cpu
from conftest import ROOT, pkg

F0 = 0.5e6


def test_one_point_source_is_a_one_element_array():
    src = pkg("sources")
    T = 1.0 / F0
    for kw in (dict(), dict(amplitude=2.5, phase=-1.1, delay=0.7 * T), dict(amplitude=0.3, phase=2.0, delay=1.5 * T, duration=11 * T)):
        ps = src.PointSources([0.001, 0.002, 0.003], **kw)
        arr = src.SourceArray([0], n_elements=1, **kw)
        for t in np.concatenate([np.linspace(0.0, 16 * T, 301), [0.7 * T, 1.5 * T, 4 * T, 12.5 * T]]):
            for scale in (1.0, 7.0):
                g, dg = ps.values(t, F0, scale)
                ga, dga = arr.values(t, F0, scale)
                assert g.shape == (1,) and g[0] == ga[0] and dg[0] == dga[0]
        assert ps.stage_scalars(2e-6, F0, 1.0).tolist() == arr.stage_scalars(2e-6, F0, 1.0).tolist()
    # several points: each its own waveform; the default scale is 1 (the amplitude is the monopole strength)
    ps = src.PointSources(np.zeros((3, 3)), amplitude=[1.0, 2.0, 0.0], phase=[0.0, 0.5, 1.0], delay=[0.0, T, 2 * T])
    g, _ = ps.values(6.3 * T, F0)
    assert g.shape == (3,) and g[2] == 0.0 and abs(g[0] - np.cos(2 * np.pi * 6.3)) < 1e-12 and g[1] != g[0]
    assert src.PointSources(np.zeros((0, 3))).values(1e-6, F0)[0].shape == (0,)


def test_validation():
    src = pkg("sources")
    with pytest.raises(ValueError, match="points"):
        src.PointSources(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="finite"):
        src.PointSources([0.0, np.nan, 0.0])
    with pytest.raises(ValueError, match="amplitude"):
        src.PointSources(np.zeros((3, 3)), amplitude=[1.0, 2.0])
    with pytest.raises(ValueError, match="finite"):
        src.PointSources(np.zeros((2, 3)), delay=[0.0, np.inf])
    with pytest.raises(ValueError, match="duration"):
        src.PointSources(np.zeros((2, 3)), duration=-1.0)
    with pytest.raises(ValueError, match="shorter"):
        src.PointSources(np.zeros((1, 3)), duration=7 / F0).check_duration(F0)


def test_claim_points_lowest_rank_holds():
    """Two split-x ranks: a point on the interface plane lies in cells of both and is claimed by rank 0 alone; one that no rank holds
    is an error, not a silent drop."""
    boxmesh, src, sensors = pkg("boxmesh"), pkg("sources"), pkg("sensors")
    L = 0.012
    meshes = [boxmesh.BoxMesh(2, (4, 2, 2), grid=(2, 1, 1), rank=r, length=L) for r in range(2)]
    pts = np.array([[0.5 * L, 0.3 * L, 0.3 * L], [0.8 * L, 0.6 * L, 0.2 * L], [0.1 * L, 0.1 * L, 0.9 * L]])
    setups = [sensors.sensor_setup(m, pts) for m in meshes]
    assert 0 in setups[0].point_ids and 0 in setups[1].point_ids
    claims = src.claim_points(setups, 3)
    assert [c.tolist() for c in claims] == [[True, False, True], [False, True, False]]
    assert np.array_equal(sum(c.astype(int) for c in claims), np.ones(3, dtype=int))
    with pytest.raises(ValueError, match="outside"):
        src.claim_points(setups, 4)


def test_host_model_is_the_adjoint_of_interpolation():
    """tests/point_source_cpu.inject against the interpolant of the same set-up: sum_j inject(q)[j] x[j] == sum_p q_p x(point p)."""
    boxmesh, sensors = pkg("boxmesh"), pkg("sensors")
    mesh = boxmesh.BoxMesh(3, (3, 2, 2), length=0.01, perturb=0.1, seed=1)
    rng = np.random.default_rng(0)
    pts = rng.uniform(0.001, 0.009, (7, 3))
    su = sensors.sensor_setup(mesh, pts)
    x, q = rng.standard_normal(mesh.ndofs), rng.standard_normal(7)
    b = point_source_cpu.inject(np.zeros(mesh.ndofs), su, q[su.point_ids], 4)
    probe = np.array([(np.einsum("i,j,k->ijk", *su.weights[p]).reshape(-1) * x[su.rows[su.cell_index[p]]]).sum() for p in range(7)])
    assert abs(b @ x - q[su.point_ids] @ probe) < 1e-12 * np.abs(b).sum() * np.abs(x).max()


def test_abi_argument_checks_precede_device_work():
    lib = pkg("_lib").load()
    z = C.c_void_p(0)
    one = C.c_void_p(256)  # non-null, never dereferenced: validation fails first
    stage = (C.c_double * 6)(0.0, 2 * np.pi * 5e5, 1.0, 5e5, 4.0, 0.0)
    sp = C.cast(stage, C.c_void_p)
    for suf in ("f64", "f32"):
        fn = getattr(lib, f"fus_point_source_{suf}")

        def call(y=one, cells=one, m=1, rows=one, k=1, w=one, P=3, a=one, ph=one, tau=one, st=sp):
            return fn(y, cells, m, rows, k, w, P, a, ph, tau, st, z)

        assert call(y=z, cells=z, m=0, rows=z, k=0, w=z, a=z, ph=z, tau=z, st=z) == 0  # zero points: a no-op
        assert call(m=-1) == -1 and call(k=-1) == -1
        assert call(P=0) == -2 and call(P=11) == -2
        for name in ("y", "cells", "rows", "w", "a", "ph", "tau", "st"):
            assert call(**{name: z}) == -1, name
        for name in ("a", "ph", "tau", "st"):
            assert call(**{name: C.c_void_p(260)}) == -1, name  # fp64 tables not 8-byte aligned
        assert call(cells=C.c_void_p(258)) == -1 and call(rows=C.c_void_p(258)) == -1
        for bad in ((3, 0.0), (4, 0.0), (5, -1.0), (3, float("nan"))):
            st2 = (C.c_double * 6)(*stage)
            st2[bad[0]] = bad[1]
            assert call(st=C.cast(st2, C.c_void_p)) == -1, bad


def test_declared_and_bound():
    """The four entry points are declared in include/fus_gpu_array.h (the extension header; include/fus_gpu.h keeps its pinned set of
    functions), bound from it with the header's types, exported by the library, and the ABI version stays 3."""
    lib_mod = pkg("_lib")
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    hdr = open(os.path.join(ROOT, "include", "fus_gpu_array.h")).read()
    names = ("fus_point_source_f64", "fus_point_source_f32", "fus_element_receive_f64", "fus_element_receive_f32")
    assert set(lib_mod.EXTENSIONS) == set(names) and not set(names) & set(lib_mod.DECLARATIONS)
    lib = lib_mod.load()
    for name in names:
        restype, argtypes = lib_mod.EXTENSIONS[name]
        fn = getattr(lib, name)
        assert re.search(rf"\b{name}\s*\(", hdr) and restype is i and fn.restype is i and list(fn.argtypes) == argtypes
    assert lib_mod.EXTENSIONS["fus_point_source_f64"][1] == [vp, vp, i64, vp, i64, vp, i, vp, vp, vp, vp, vp]
    assert lib_mod.EXTENSIONS["fus_element_receive_f32"][1] == [vp, vp, vp, vp, i64, vp, i64, i, vp, vp, vp, i, vp]
    assert '#include "fus_gpu_array.h"' in open(os.path.join(ROOT, "include", "fus_gpu.hpp")).read()
    assert lib_mod.ABI_VERSION == 3 and lib.fus_abi_version() == 3


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_point_source_kernel_resource_pin():
    """The launch runs next to a chip-filling stiffness launch: no scratch, no AGPRs, at most 64 VGPRs, at least 8 waves per SIMD, at
    every instantiated degree and for both types."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    table = ru.parse(ru.cached_remarks())
    for T in ("double", "float"):
        hits = [(k, v) for k, v in table.items() if re.search(rf"point_source_kernel<{T}, \d+>", k)]
        assert len(hits) == 10, hits
        for k, d in hits:
            assert d["scratch"] == 0 and d["agpr"] == 0 and d["vgpr"] <= 64 and d["occupancy"] >= 8 and d["lds"] == 0, (k, d)
