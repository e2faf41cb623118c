"""What tests/test_small_kernels_gpu.py takes for granted about tests/geometry_model.py, on the CPU: the longdouble model is the host
precompute and the reference's golden outputs; mirroring a cell changes nothing; every family has the features its name states; and
the inputs are well conditioned: the restatement of the kernel in its own type stays within 32 units of the model."""

import numpy as np
import pytest

import geometry_model as gm
from conftest import golden_files, pkg, rel_l2

DTYPES = [np.float64, np.float32]
NCELL = 300


def _case(family, nq, dtype, ncell=NCELL):
    x_dofs, x_g = gm.cells(family, ncell, dtype)
    dphi, w = gm.rule(nq, dtype)
    return x_dofs, x_g, dphi, w


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("family", gm.FAMILIES)
def test_model_equals_host_precompute(family, dtype):
    """``precompute`` evaluates the same formulas in fp64 in another order (einsum, inverse before the product): on inputs whose own
    restatement is held to 32 units it stays within 64 units of 2^-53 of the model, per (cell, q)."""
    pre = pkg("precompute")
    u = 64 * 2.0**-53
    for nq, nqf in ((7, 4), (27, 9)):
        x_dofs, x_g, dphi, w = _case(family, nq, dtype)
        Gm, dm = gm.model(x_dofs, x_g, dphi, w)
        G, d = np.zeros((NCELL, nq, 6)), np.zeros((NCELL, nq))
        pre.compute_scaled_geometrical_factor(G, (x_dofs, x_g), NCELL, dphi, w)
        pre.compute_scaled_jacobian_determinant(d, (x_dofs, x_g), NCELL, dphi, w)
        assert gm.g_errors(G, Gm)[0] <= u and gm.det_errors(d, dm)[0] <= u
        dphi_f, wf = gm.facet_rule(nqf, dtype)
        bd = gm.boundary(NCELL, 500)
        dF = np.zeros((500, nqf))
        pre.compute_boundary_facets_scaled_jacobian_determinant(dF, (x_dofs, x_g), bd, dphi_f, wf)
        assert gm.det_errors(dF, gm.facet_model(x_dofs, x_g, bd, dphi_f, wf))[0] <= u


@pytest.mark.parametrize("path", golden_files("ops_"), ids=lambda p: p.split("/")[-1][:-4])
def test_model_equals_the_golden_outputs(path):
    """The bounds of tests/test_precompute.py."""
    d = np.load(path)
    tol = 2e-15 if d["x"].dtype == np.float64 else 2e-6
    G, detJ = gm.model(d["x_dofs"], d["x_g"], d["dphi_geom"], d["wts3"])
    dF = gm.facet_model(d["x_dofs"], d["x_g"], d["boundary_data"], d["dphi_facet"], d["wts2"])
    assert rel_l2(G, d["ref_G"]) < tol and rel_l2(detJ, d["ref_detJ"]) < tol and rel_l2(dF, d["ref_detJ_f"]) < tol


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_mirroring_a_cell_changes_no_output(dtype):
    """x -> -x negates one column of J_ exactly: G, detJ and detJ_f keep every bit, in the model and in the restatement."""
    x_dofs, x_g, dphi, w = _case("sheared", 27, dtype, 64)
    dphi_f, wf = gm.facet_rule(9, dtype)
    bd = gm.boundary(64, 200)
    xm = x_g.copy()
    xm[:, 0] *= -1
    for ev, fev in ((gm.model, gm.facet_model), (gm.restate, gm.facet_restate)):
        (G, d), (G2, d2) = ev(x_dofs, x_g, dphi, w), ev(x_dofs, xm, dphi, w)
        assert np.array_equal(G, G2) and np.array_equal(d, d2)
        assert np.array_equal(fev(x_dofs, x_g, bd, dphi_f, wf), fev(x_dofs, xm, bd, dphi_f, wf))


def test_the_families_are_what_their_names_state():
    for family, f in gm.FAMILIES.items():
        X = gm.cell_coordinates(family, 50)
        e = X[:, [1, 2, 4]] - X[:, [0]]  # the three edges at vertex 0: [c, a, d]
        det = np.linalg.det(e)
        assert np.all(det[0::2] > 0) and np.all((det[1::2] < 0) == f["mirror"])
        off = np.abs(e[:, [0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 0, 1]])
        assert np.all(off == 0) if not f["shear"] else np.all(off.max(axis=1) > 0.01 * f["h"])
        assert np.all(np.abs(det) > 0.1 * f["h"] ** 3)
        # vertices are numbered through a permutation: neither monotone nor block-wise
        x_dofs, x_g = gm.cells(family, 50, np.float64)
        assert sorted(x_dofs.reshape(-1)) == list(range(400)) and np.any(np.diff(x_dofs.reshape(-1)) < 0)
        assert np.any(x_dofs.max(axis=1) - x_dofs.min(axis=1) > 8)
        assert np.array_equal(x_g[x_dofs], X)
    # the periodic form: cell c has the coordinates of cell c mod period, on vertices of its own
    x_dofs, x_g = gm.cells("mirrored", 41, np.float64, period=7)
    assert np.array_equal(x_g[x_dofs][7:14], x_g[x_dofs][:7]) and np.unique(x_dofs).size == 8 * 41
    bd = gm.boundary(50, 100)
    assert set(bd[:, 1]) == set(range(6)) and np.any(np.diff(bd[:, 0]) < 0) and np.unique(bd[:, 0]).size < 100
    for nq in gm.NQ:
        dphi, w = gm.rule(nq, np.float64)
        assert dphi.shape == (3, nq, 8) and w.min() >= 0.1 and w.max() <= 1.1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("family", gm.FAMILIES)
def test_the_inputs_are_well_conditioned(family, dtype):
    """e_cpu, the restatement in T against the model, is at most 32 units (2^-24 fp32, 2^-53 fp64) in the maximum: the condition that
    keeps the GPU bar of 8 x e_cpu from going slack."""
    unit = gm.UNIT[np.dtype(dtype)]
    for nq, nqf in zip(gm.NQ, gm.NQF):
        ncell = NCELL if nq < 1331 else 40
        x_dofs, x_g, dphi, w = _case(family, nq, dtype, ncell)
        (G, d), (Gm, dm) = gm.restate(x_dofs, x_g, dphi, w), gm.model(x_dofs, x_g, dphi, w)
        dphi_f, wf = gm.facet_rule(nqf, dtype)
        bd = gm.boundary(ncell, 500)
        eF = gm.det_errors(gm.facet_restate(x_dofs, x_g, bd, dphi_f, wf), gm.facet_model(x_dofs, x_g, bd, dphi_f, wf))
        eG, eD = gm.g_errors(G, Gm), gm.det_errors(d, dm)
        print(f"{family} nq {nq} nqf {nqf}: G {eG[0] / unit:.1f} (rms {eG[1] / unit:.1f}) detJ {eD[0] / unit:.1f} detJ_f {eF[0] / unit:.1f} units")
        assert 0 < eG[0] <= gm.E_CPU_CAP * unit and 0 < eD[0] <= gm.E_CPU_CAP * unit and 0 < eF[0] <= gm.E_CPU_CAP * unit
