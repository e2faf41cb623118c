"""Element receivers on the host (receivers.py): the CSR layout of a receiving array, the merge of partitioned ranks' partial integrals
and areas, time_reversal on synthetic harmonics, the C ABI's argument checks of fus_element_receive_* (no device work) and the
resource pin of the kernel."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import point_source_cpu
from conftest import ROOT, pkg
from oracle import rk4_oracle
from test_sources import _array_mesh


def _layout(mesh, fn, E):
    src, rx = pkg("sources"), pkg("receivers")
    bd = mesh.boundary_facets([getattr(mesh, "source_tag", 2)])
    ids = src.SourceArray(fn, n_elements=E).assign(mesh, bd)
    fdm, dF = mesh.facet_dofmap(bd), rk4_oracle.host_facet_detJ(mesh, bd)
    return ids, fdm, dF, rx.element_entries(ids, fdm, dF, E)


def test_csr_layout_on_box_and_array_mesh():
    """Entries sorted by element, offsets from the counts, an element without facets empty; on a cell-permuted ArrayMesh the same
    callable gives every element the same multiset of weights; and the CSR sums are the numpy receiver's."""
    src = pkg("sources")
    box, am = _array_mesh()
    fn = src.grid_elements(3, 2, (0.0, 0.01), (0.0, 0.01))
    E = 8  # elements 6 and 7 have no facets
    rng = np.random.default_rng(2)
    per_mesh = []
    for mesh in (box, am):
        ids, fdm, dF, (dof, wgt, offs) = _layout(mesh, fn, E)
        n2 = fdm.shape[1]
        assert dof.dtype == np.int32 and offs.dtype == np.int64 and offs.shape == (E + 1,) and offs[0] == 0
        assert np.array_equal(np.diff(offs), np.bincount(ids, minlength=E) * n2) and offs[-1] == dof.size == wgt.size
        assert offs[6] == offs[7] == offs[8]
        for e in range(E):  # stable: facet order, then the facet's local order
            assert np.array_equal(dof[offs[e]:offs[e + 1]], fdm[ids == e].reshape(-1))
            assert np.array_equal(wgt[offs[e]:offs[e + 1]], dF[ids == e].reshape(-1))
        u = rng.standard_normal(mesh.ndofs)
        S, A = point_source_cpu.receive(u, ids, fdm, dF, E)
        got = np.array([(wgt[offs[e]:offs[e + 1]] * u[dof[offs[e]:offs[e + 1]]]).sum() for e in range(E)])
        assert np.allclose(got, S, rtol=1e-13, atol=1e-20) and A[6] == 0.0
        per_mesh.append([np.sort(wgt[offs[e]:offs[e + 1]]) for e in range(E)])
    for a, b in zip(*per_mesh):  # the same facets, whatever their order: the same multiset of weights per element
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-12, atol=0.0)


def test_inactive_facets_and_shape_checks():
    rx = pkg("receivers")
    ids = np.array([1, -1, 0, 1])
    fdm = np.arange(12).reshape(4, 3)
    dof, wgt, offs = rx.element_entries(ids, fdm, fdm * 0.5, 3)
    assert dof.tolist() == [6, 7, 8, 0, 1, 2, 9, 10, 11] and offs.tolist() == [0, 3, 9, 9] and wgt.tolist() == (dof * 0.5).tolist()
    with pytest.raises(ValueError, match="shape"):
        rx.element_entries(ids, fdm, np.zeros((4, 2)), 3)


def test_merge_of_split_y_ranks_equals_serial_average():
    """Two split-y ranks cut every element of a 1 x 4 array (strips along y) in two: partial integrals and partial areas add to the serial ones, and
    the area average of the merged parts equals the serial average (a rank's own average would not)."""
    boxmesh, src, rx = pkg("boxmesh"), pkg("sources"), pkg("receivers")
    P, cells, L, E = 3, (2, 4, 4), 0.012, 5  # element 4 exists on no rank
    fn = src.grid_elements(1, 4, (0.0, L), (0.0, L))
    serial = boxmesh.BoxMesh(P, cells, length=L, perturb=0.1, seed=6)
    field = lambda xyz: np.sin(310.0 * xyz[:, 1] + 1.0) * np.cos(170.0 * xyz[:, 2]) + 0.3  # noqa: E731
    ids, fdm, dF, _ = _layout(serial, fn, E)
    S1, A1 = point_source_cpu.receive(field(serial.dof_coordinates()), ids, fdm, dF, E)
    parts = []
    for r in range(2):
        m = boxmesh.BoxMesh(P, cells, grid=(1, 2, 1), rank=r, length=L, perturb=0.1, seed=6)
        ids_r, fdm_r, dF_r, _ = _layout(m, fn, E)
        S, A = point_source_cpu.receive(field(m.dof_coordinates()), ids_r, fdm_r, dF_r, E)
        assert np.all(A[:4] > 0) and np.all(A[:4] < A1[:4])  # every element has a part on each rank
        parts.append((A, np.stack([S, 2.0 * S])))  # two "records"
    merged = rx.merge(parts)
    assert merged.shape == (2, E) and np.all(np.isnan(merged[:, 4]))
    assert np.allclose(sum(a for a, _ in parts), A1, rtol=1e-13)
    assert np.allclose(merged[0, :4], (S1[:4] / A1[:4]), rtol=1e-12) and np.allclose(merged[1, :4], 2 * (S1[:4] / A1[:4]), rtol=1e-12)
    # complex sums merge alike
    c = rx.merge([(a, v[0] * (1 + 2j)) for a, v in parts])
    assert np.allclose(c[:4], (S1[:4] / A1[:4]) * (1 + 2j), rtol=1e-12)
    with pytest.raises(ValueError):
        rx.merge([(parts[0][0], np.zeros(3))])


def test_time_reversal_on_synthetic_harmonics():
    rx, src = pkg("receivers"), pkg("sources")
    fn = src.grid_elements(2, 3, (0.0, 1.0), (0.0, 1.0))
    mag = np.array([2.0, 0.5, 1.0, 0.0, 4.0, 1.5])
    ang = np.array([0.3, -2.9, np.pi, 1.0, -np.pi, 3.1])
    R = mag * np.exp(1j * ang)
    arr = rx.time_reversal(R, element_of_facet=fn)
    assert isinstance(arr, src.SourceArray) and arr.n_elements == 6 and arr.element_of_facet is fn and arr.duration is None
    heard = mag > 0
    # conjugate phases: R_e e^{i phase_e} is real and positive for every element that received something
    assert np.allclose(np.angle(R[heard] * np.exp(1j * arr.phase[heard])), 0.0, atol=1e-12)
    assert np.all(arr.phase > -np.pi) and np.all(arr.phase <= np.pi)
    assert arr.phase[2] == np.pi and arr.phase[4] == np.pi  # -arg = -pi and +pi both wrap to +pi, never -pi
    assert arr.phase[3] == 0.0 and arr.amplitude[3] == 0.0  # an element that received nothing stays silent
    assert arr.amplitude.tolist() == [1.0, 1.0, 1.0, 0.0, 1.0, 1.0]
    conj = rx.time_reversal(R, amplitude="conjugate", duration=2e-5, element_of_facet=fn)
    assert np.allclose(conj.amplitude, mag / 4.0) and conj.duration == 2e-5 and np.array_equal(conj.phase, arr.phase)
    nan = R.copy()
    nan[1] = np.nan
    assert rx.time_reversal(nan, element_of_facet=fn).amplitude[1] == 0.0
    with pytest.raises(ValueError, match="amplitude"):
        rx.time_reversal(R, amplitude="loud", element_of_facet=fn)
    with pytest.raises(ValueError, match="element_of_facet"):
        rx.time_reversal(R)
    with pytest.raises(ValueError, match="received"):
        rx.time_reversal(np.zeros(3, complex), element_of_facet=fn)


def test_abi_argument_checks_precede_device_work():
    lib = pkg("_lib").load()
    z = C.c_void_p(0)
    one = C.c_void_p(256)  # non-null, never dereferenced: validation fails first
    for suf in ("f64", "f32"):
        fn = getattr(lib, f"fus_element_receive_{suf}")

        def call(u=one, dof=one, wgt=one, offs=one, E=1, rec=z, cap=0, slot=0, hre=z, him=z, coef=z, H=0):
            return fn(u, dof, wgt, offs, E, rec, cap, slot, hre, him, coef, H, z)

        assert call(u=z, dof=z, wgt=z, offs=z, E=0) == 0  # no elements: a no-op
        assert call(E=-1) == -1 and call(cap=-1) == -1 and call(H=-1) == -1
        for name in ("u", "dof", "wgt", "offs"):
            assert call(**{name: z}) == -1, name
        assert call(rec=one, cap=2, slot=2) == -1 and call(rec=one, cap=2, slot=-1) == -1 and call(rec=one, cap=0) == -1
        assert call(hre=one, him=one, coef=one, H=0) == -1 and call(H=1) == -1 and call(hre=one, him=z, coef=one, H=1) == -1
        assert call(hre=one, him=one, coef=z, H=1) == -1
        assert call(offs=C.c_void_p(260)) == -1 and call(dof=C.c_void_p(258)) == -1  # int64 offsets, int32 dofs
        for name in ("hre", "him", "coef"):  # fp64 tables not 8-byte aligned
            assert call(**{**dict(hre=one, him=one, coef=one, H=1), name: C.c_void_p(260)}) == -1, name


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_element_receive_kernel_resource_pin():
    """No scratch, no AGPRs, at most 64 VGPRs, at least 8 waves per SIMD, and only the four wave partials in LDS, for both types."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    table = ru.parse(ru.cached_remarks())
    for T in ("double", "float"):
        hits = [(k, v) for k, v in table.items() if re.search(rf"element_receive_kernel<{T}>", k)]
        assert len(hits) == 1, hits
        d = hits[0][1]
        assert d["scratch"] == 0 and d["agpr"] == 0 and d["vgpr"] <= 64 and d["occupancy"] >= 8 and d["lds"] == 32, (T, d)
