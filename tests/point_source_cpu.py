"""Host model of point sources and element receivers (test infrastructure): the monopole term as a ``source_term`` hook of
``oracle.rk4_oracle.solve`` / ``solve_westervelt`` -- the hook that receives the stage's source time -- and a numpy receiver.

The hook REPLACES the model's facet source: ``facet_scale`` adds the uniform source itself for a "both sources" case."""

import numpy as np

from conftest import pkg


def inject(b, setup, q, n):
    """b[rows[cell_index[p]][ijk]] += q[p] Lx[i] Ly[j] Lz[k] for the points of a ``SensorSetup`` (np.add.at: points may share dofs)."""
    for p in range(setup.point_ids.size):
        lx, ly, lz = setup.weights[p]
        w = (lx[:, None, None] * ly[None, :, None] * lz[None, None, :]).reshape(-1)
        np.add.at(b, setup.rows[setup.cell_index[p]], q[p] * w)
    return b


def point_term(mesh, points, f0, facet_scale=None):
    """``source_term(t, b, coefficients, detJ, dofmap)``: the points of ``points`` (a ``sources.PointSources``) at time ``t``; with
    ``facet_scale = (A, alpha)`` also the uniform facet source ``A W(t) cos(w0 t)`` of the linear model."""
    setup = pkg("sensors").sensor_setup(mesh, points.points)
    assert setup.point_ids.size == points.npoints, "a point lies outside the mesh"
    n = mesh.P + 1

    def term(t, b, coefficients, detJ, dofmap):
        g, _ = points.values(t, f0)
        inject(b, setup, g[setup.point_ids], n)
        if facet_scale is not None:
            A, alpha = facet_scale
            window = 0.5 * (1 - np.cos(f0 * np.pi * t / alpha)) if t < alpha / f0 else 1.0
            np.add.at(b, dofmap, window * A * np.cos(2 * np.pi * f0 * t) * coefficients[0][:, None] * detJ)

    return term


def receive(u, ids, facet_dofmap, facet_detJ, n_elements):
    """``(S [E], A [E])``: the integrals sum detJ u over the facets of each element and the elements' areas."""
    ids = np.asarray(ids)
    act = ids >= 0
    S = np.bincount(ids[act], weights=(facet_detJ[act] * np.asarray(u, dtype=np.float64)[facet_dofmap[act]]).sum(axis=1), minlength=n_elements)
    A = np.bincount(ids[act], weights=facet_detJ[act].sum(axis=1), minlength=n_elements)
    return S, A
