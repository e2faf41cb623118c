"""CPU model of the sponge layer for the tests: the two loops of ``oracle/rk4_oracle.py`` (``solve`` / ``solve_westervelt``) restated
statement for statement in numpy on the same oracle operators, with the layer's term in the right-hand side of every stage,

    b -= cv * vn + cu * un,        cv = 2 sigma m,  cu = sigma^2 m        (m: the lumped mass; the Westervelt loop's m0)

before ``b / m``.  With sigma == 0 both return what the oracle's loops return, bitwise (tests/test_sponge.py).  Optional: an initial
state ``(u, v)``, a switch that drops every boundary-facet term, and the factors of the two coefficients (the wrong forms the
constant-sigma identity must tell apart).  One rank.  Not a test module."""

import numpy as np

from conftest import pkg
from oracle import oracle_np
from oracle.rk4_oracle import A, B, C


def _geometry(mesh):
    gll, pre = pkg("gll"), pkg("precompute")
    P, n, nc = mesh.P, mesh.P + 1, mesh.ncells
    pts, wts, D = gll.tabulate_1d(P)
    w3 = gll.tensor_weights_3d(wts)
    dg = pre.tabulate_hex_p1_gradients(gll.tensor_points_3d(pts))
    bd1, bd2 = mesh.boundary_facets([2]), mesh.boundary_facets([3])
    G, detJ = np.zeros((nc, n**3, 6)), np.zeros((nc, n**3))
    pre.compute_scaled_geometrical_factor(G, (mesh.x_dofs, mesh.x_g), nc, dg, w3)
    pre.compute_scaled_jacobian_determinant(detJ, (mesh.x_dofs, mesh.x_g), nc, dg, w3)
    w2, dpf = gll.tensor_weights_2d(wts), pre.tabulate_facet_gradients(pts)
    dF1, dF2 = np.zeros((bd1.shape[0], n * n)), np.zeros((bd2.shape[0], n * n))
    pre.compute_boundary_facets_scaled_jacobian_determinant(dF1, (mesh.x_dofs, mesh.x_g), bd1, dpf, w2)
    pre.compute_boundary_facets_scaled_jacobian_determinant(dF2, (mesh.x_dofs, mesh.x_g), bd2, dpf, w2)
    return D, G, detJ, bd1, bd2, dF1, dF2, mesh.facet_dofmap(bd1), mesh.facet_dofmap(bd2)


def _sigma(mesh, sigma):
    """sigma as one value per dof of the (single-rank) mesh: None, a scalar, an array, or a callable of the dof coordinates."""
    if sigma is None:
        return np.zeros(mesh.ndofs)
    if callable(sigma):
        return np.asarray(sigma(mesh.dof_coordinates()), dtype=np.float64)
    return np.broadcast_to(np.asarray(sigma, dtype=np.float64), (mesh.ndofs,)).copy()


def _rk4(f1, nd, nsteps, dt, source_time, u, v):
    u = np.zeros(nd) if u is None else np.array(u, dtype=np.float64)
    v = np.zeros(nd) if v is None else np.array(v, dtype=np.float64)
    ku, kv = np.zeros(nd), np.zeros(nd)
    t = 0.0
    for dt in (list(dt) if hasattr(dt, "__len__") else [dt] * nsteps):
        u0, v0 = u.copy(), v.copy()
        for i in range(4):
            un = u0 + A[i] * dt * ku
            vn = v0 + A[i] * dt * kv
            tn = t + C[i] * dt
            ku = vn.copy()
            kv = f1(tn if source_time == "tn" else t, un, vn)
            u = u + B[i] * dt * ku
            v = v + B[i] * dt * kv
        t += dt
    return u, v


def solve(mesh, nsteps, dt, sigma=None, c0=1500.0, rho0=1000.0, f0=0.5e6, p0=60000.0, source_time="tn", oracle_c=None, u=None, v=None,
          facets=True, cv_factor=2.0, cu_factor=1.0):
    """``rk4_oracle.solve`` (homogeneous medium) with the layer.  ``oracle_c``: the C restatement of the operators."""
    P = mesh.P
    D, G, detJ, bd1, bd2, dF1, dF2, fd1, fd2 = _geometry(mesh)
    nc, nd = mesh.ncells, mesh.ndofs
    c_, rho_ = np.full(nc, float(c0)), np.full(nc, float(rho0))
    cc1, cc2 = 1 / rho_ / c_ / c_, -1 / rho_
    fc1, fc2 = 1 / rho_[bd1[:, 0]], -1 / rho_[bd2[:, 0]] / c_[bd2[:, 0]]
    w0 = 2 * np.pi * f0
    m = np.zeros(nd)
    mass = oracle_c.mass_apply if oracle_c is not None else oracle_np.mass_apply
    mass(np.ones(nd), cc1, m, detJ, mesh.dofmap)
    sig = _sigma(mesh, sigma)
    cv, cu = cv_factor * sig * m, cu_factor * (sig * sig) * m

    def stiff(x, y):
        if oracle_c is not None:
            oracle_c.stiffness_apply(P, D, x, cc2, y, G, mesh.dofmap)
        else:
            oracle_np.stiffness_apply(P, D.flatten(), x, cc2, y, G, mesh.dofmap)

    def f1(t, un, vn):
        T, alpha = 1 / f0, 4.0
        window = 0.5 * (1 - np.cos(f0 * np.pi * t / alpha)) if t < T * alpha else 1.0
        g = np.full(nd, window * p0 * w0 / c0 * np.cos(w0 * t))
        b = np.zeros(nd)
        stiff(np.ascontiguousarray(un), b)
        if facets:
            mass(g, fc1, b, dF1, fd1)
            mass(np.ascontiguousarray(vn), fc2, b, dF2, fd2)
        b -= cv * vn + cu * un
        return b / m

    return _rk4(f1, nd, nsteps, dt, source_time, u, v)


def solve_westervelt(mesh, nsteps, dt, sigma=None, c0=1480.0, rho0=1000.0, f0=1.1e6, p0=None, beta=3.5, att_dB=0.2, source_time="tn",
                     oracle_c=None, u=None, v=None, facets=True, cv_factor=2.0, cu_factor=1.0):
    """``rk4_oracle.solve_westervelt`` (homogeneous medium) with the layer: its coefficients carry the steady lumped mass m0."""
    P = mesh.P
    D, G, detJ, bd1, bd2, dF1, dF2, fd1, fd2 = _geometry(mesh)
    c_ref, rho_ref = float(c0), float(rho0)
    if p0 is None:
        p0 = rho_ref * c_ref * 0.38557513826589934
    w0 = 2 * np.pi * f0
    c0, rho0, beta, att_dB = (np.broadcast_to(np.asarray(a, dtype=np.float64), (mesh.ncells,)).copy() for a in (c0, rho0, beta, att_dB))
    delta = 2 * (att_dB / 20 * np.log(10)) * c0**3 / w0 / w0
    cc1 = 1 / rho0 / c0**2
    cc2 = -2 * beta / rho0**2 / c0**4
    cc3 = -1 / rho0
    cc4 = -delta / rho0 / c0**2
    cc5 = 2 * beta / rho0**2 / c0**4
    i1, i2 = bd1[:, 0], bd2[:, 0]
    f11, f21 = 1 / rho0[i1], delta[i1] / rho0[i1] / c0[i1] ** 2
    f12, f22 = delta[i2] / rho0[i2] / c0[i2] ** 3, -1 / rho0[i2] / c0[i2]
    c0 = c_ref
    nd = mesh.ndofs
    ones = np.ones(nd)
    m0 = np.zeros(nd)
    mass_apply = oracle_np.mass_apply
    oracle_np.mass_apply(ones, cc1, m0, detJ, mesh.dofmap)
    if facets:
        oracle_np.mass_apply(ones, f12, m0, dF2, fd2)
    sig = _sigma(mesh, sigma)
    cv, cu = cv_factor * sig * m0, cu_factor * (sig * sig) * m0

    def stiff(x, cc, y):
        if oracle_c is not None:
            oracle_c.stiffness_apply(P, D, x, cc, y, G, mesh.dofmap)
        else:
            oracle_np.stiffness_apply(P, D.flatten(), x, cc, y, G, mesh.dofmap)

    def f1(t, un, vn):
        T, alpha = 1 / f0, 4.0
        if t < T * alpha:
            window = 0.5 * (1 - np.cos(f0 * np.pi * t / alpha))
            dwindow = 0.5 * np.pi * f0 / alpha * np.sin(f0 * np.pi * t / alpha)
        else:
            window, dwindow = 1.0, 0.0
        a = 2 * p0 * w0 / c0
        g = np.full(nd, window * a * np.cos(w0 * t))
        dg = np.full(nd, dwindow * a * np.cos(w0 * t) - window * a * w0 * np.sin(w0 * t))
        m = np.zeros(nd)
        mass_apply(np.ascontiguousarray(un), cc2, m, detJ, mesh.dofmap)
        m += m0
        b = np.zeros(nd)
        stiff(np.ascontiguousarray(un), cc3, b)
        stiff(np.ascontiguousarray(vn), cc4, b)
        mass_apply(vn * vn, cc5, b, detJ, mesh.dofmap)
        if facets:
            mass_apply(g, f11, b, dF1, fd1)
            mass_apply(dg, f21, b, dF1, fd1)
            mass_apply(np.ascontiguousarray(vn), f22, b, dF2, fd2)
        b -= cv * vn + cu * un
        return b / m

    return _rk4(f1, nd, nsteps, dt, source_time, u, v)
