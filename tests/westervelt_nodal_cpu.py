"""The Westervelt solver with a nodal medium in the CPU wave model, for the tests.  As tests/nodal_cpu.py: the operators are the
oracle's own.  The stiffness part of a stage is ``oracle_np.stiffness_apply`` on ``G kappa3[dofmap]`` for u plus
``G kappa4[dofmap]`` for v (kappa3 = 1/rho, kappa4 = delta/(rho c^2), cell constants -1); the three diagonals are ONE unit-coefficient
mass apply times nodal factors,

    m0 = M(1)1 / (rho c^2) + the facet term,    w2 = M(1)1 (-2 beta / (rho^2 c^4)),    w5 = -w2,

and the facet rule keeps one coefficient per facet: the mean over the facet's dofs of the nodal expression.  The hooks are those of
``rk4_oracle.solve_westervelt`` (``stage_term``: tests/sponge_cpu.py; ``source_term``: tests/point_source_cpu.py); with
``relaxation=(tau, kappa)`` (scalar weights) the loop over ``(u, v, xi)`` is tests/relaxation_cpu.py's, K(kappa3) acting on
``u_n + sum xi``.  One rank.  Not a test module."""

import numpy as np

import relaxation_cpu
from nodal_cpu import scaled_G
from oracle import oracle_np, rk4_oracle


def diffusivity(w0, c, att_dB):
    """compute_diffusivity_of_sound at the angular frequency ``w0``."""
    return 2 * (np.asarray(att_dB) / 20 * np.log(10)) * np.asarray(c) ** 3 / w0 / w0


def stiffness_pair(P, D, u, v, c3, c4, b, G, dofmap, kappa3, kappa4):
    """b += K(c3 kappa3) u + K(c4 kappa4) v."""
    Df = np.asarray(D).flatten()
    oracle_np.stiffness_apply(P, Df, np.ascontiguousarray(u), c3, b, scaled_G(G, kappa3, dofmap), dofmap)
    oracle_np.stiffness_apply(P, Df, np.ascontiguousarray(v), c4, b, scaled_G(G, kappa4, dofmap), dofmap)


def solve(mesh, nsteps, dt, c_nodal, rho_nodal, beta_nodal, att_nodal, f0=1.1e6, p0=None, source_time="tn", c_ref=None, rho_ref=None,
          stage_term=None, source_term=None, relaxation=None, record=None):
    """``(u, v)`` after ``nsteps`` steps (``(u, v, xi)`` with ``relaxation=(tau, kappa)``, which also takes ``record(t, u, v)``).  Each
    nodal field: one value per dof, or a scalar."""
    D, G, detJ, bd1, bd2, dF1, dF2, fd1, fd2 = rk4_oracle.host_geometry(mesh)
    nc, nd = mesh.ncells, mesh.ndofs
    c_, rho_, beta_, att_ = (np.broadcast_to(np.asarray(a, dtype=np.float64), (nd,)).copy() for a in (c_nodal, rho_nodal, beta_nodal, att_nodal))
    w0 = 2 * np.pi * f0
    delta_ = diffusivity(w0, c_, att_)
    c_ref = float(c_[fd1].mean()) if c_ref is None else float(c_ref)
    rho_ref = float(rho_[fd1].mean()) if rho_ref is None else float(rho_ref)
    if p0 is None:
        p0 = rho_ref * c_ref * 0.38557513826589934
    Df = D.flatten()
    G3, G4 = scaled_G(G, 1.0 / rho_, mesh.dofmap), scaled_G(G, delta_ / rho_ / c_**2, mesh.dofmap)
    minus = np.full(nc, -1.0)
    mean = lambda a, fd: a[fd].mean(axis=1) if fd.shape[0] else np.zeros(0)  # noqa: E731
    f11, f21 = mean(1.0 / rho_, fd1), mean(delta_ / rho_ / c_**2, fd1)
    f12, f22 = mean(delta_ / rho_ / c_**3, fd2), -mean(1.0 / rho_ / c_, fd2)
    ones = np.ones(nd)
    m1 = np.zeros(nd)
    oracle_np.mass_apply(ones, np.ones(nc), m1, detJ, mesh.dofmap)
    m0 = m1 / (rho_ * c_**2)
    oracle_np.mass_apply(ones, f12, m0, dF2, fd2)
    w2 = m1 * (-2.0 * beta_ / rho_**2 / c_**4)
    w5 = -w2
    term = stage_term(m0) if stage_term is not None else None

    def f1(t, ur, un, vn):
        m = m0 + w2 * un
        b = np.zeros(nd)
        oracle_np.stiffness_apply(mesh.P, Df, np.ascontiguousarray(ur), minus, b, G3, mesh.dofmap)
        oracle_np.stiffness_apply(mesh.P, Df, np.ascontiguousarray(vn), minus, b, G4, mesh.dofmap)
        b += w5 * vn * vn
        if source_term is None:
            T, alpha = 1 / f0, 4.0
            if t < T * alpha:
                window = 0.5 * (1 - np.cos(f0 * np.pi * t / alpha))
                dwindow = 0.5 * np.pi * f0 / alpha * np.sin(f0 * np.pi * t / alpha)
            else:
                window, dwindow = 1.0, 0.0
            a = 2 * p0 * w0 / c_ref
            oracle_np.mass_apply(np.full(nd, window * a * np.cos(w0 * t)), f11, b, dF1, fd1)
            oracle_np.mass_apply(np.full(nd, dwindow * a * np.cos(w0 * t) - window * a * w0 * np.sin(w0 * t)), f21, b, dF1, fd1)
        else:
            source_term(t, b, (f11, f21), dF1, fd1)
        oracle_np.mass_apply(np.ascontiguousarray(vn), f22, b, dF2, fd2)
        if term is not None:
            term(b, un, vn)
        return b / m

    dts = list(dt) if hasattr(dt, "__len__") else [dt] * nsteps
    if relaxation is None:
        assert record is None
        return rk4_oracle.rk4_loop(lambda t, un, vn: f1(t, un, un, vn), nd, dts, source_time)
    tau, kappa = relaxation
    kd = np.repeat(np.asarray(kappa, dtype=np.float64)[:, None], nd, axis=1)
    return relaxation_cpu.rk4_loop(f1, nd, dts, source_time, tau, kd, record=record)
