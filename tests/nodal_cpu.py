"""Nodal material fields in the CPU wave model, for the tests.  The operator with a nodal coefficient needs no new CPU code: it is the
oracle's own stiffness apply on the pre-scaled geometric factor,

    G'[c, q, :] = kappa[dofmap[c, q]] G[c, q, :]        (the GLL rule is collocated: kappa at the dofs is kappa at the quadrature points)

and the linear solver with a nodal medium is ``rk4_oracle.rk4_loop`` with an ``f1`` made of that apply (kappa = 1/rho, cell constant
-1), the nodal lumped mass ``(M(1) 1) * 1/(rho c^2)`` and the facet rule -- one coefficient per facet, the mean of the nodal
coefficient (1/rho on the source facets, 1/(rho c) on the absorbing ones) over the facet's dofs.  The hooks are those of
``rk4_oracle.solve`` (``stage_term``: tests/sponge_cpu.py; ``source_term``: tests/point_source_cpu.py); with ``relaxation=(tau,
kappa)`` (scalar weights) the loop over ``(u, v, xi)`` is tests/relaxation_cpu.py's.  One rank.  Not a test module."""

import numpy as np

import relaxation_cpu
from oracle import oracle_np, rk4_oracle


def scaled_G(G, kappa, dofmap):
    return G * np.asarray(kappa, dtype=G.dtype)[dofmap][:, :, None]


def stiffness_apply(P, D, x, cc, y, G, dofmap, kappa):
    """y += K(cc * kappa) x."""
    oracle_np.stiffness_apply(P, np.asarray(D).flatten(), x, cc, y, scaled_G(G, kappa, dofmap), dofmap)


def smooth_field(xyz, lo, hi, length):
    """A smooth positive field between ``lo`` and ``hi``: an oblique sine that runs through a full period over the box of edge(s)
    ``length``, so both values are (nearly) reached."""
    s = np.asarray(xyz, dtype=np.float64) / np.asarray(length, dtype=np.float64)
    w = 0.5 + 0.5 * np.sin(3.0 * (s[:, 0] + 0.7 * s[:, 1] + 0.4 * s[:, 2]) + 0.3)
    return lo + (hi - lo) * w


def lens(center, radius, base, peak):
    """``f(xyz)``: ``base`` plus a Gaussian inclusion of height ``peak - base`` at ``center``."""
    center = np.asarray(center, dtype=np.float64)

    def f(xyz):
        r2 = np.sum((np.asarray(xyz, dtype=np.float64) - center) ** 2, axis=1)
        return base + (peak - base) * np.exp(-r2 / (radius * radius))

    return f


def solve(mesh, nsteps, dt, c_nodal, rho_nodal, f0=0.5e6, p0=60000.0, source_time="tn", c_ref=None, stage_term=None, source_term=None,
          relaxation=None, record=None):
    """The linear solver with a nodal medium, ``(u, v)`` after ``nsteps`` steps (``(u, v, xi)`` with ``relaxation=(tau, kappa)``, which
    also takes ``record(t, u, v)``)."""
    D, G, detJ, bd1, bd2, dF1, dF2, fd1, fd2 = rk4_oracle.host_geometry(mesh)
    nc, nd = mesh.ncells, mesh.ndofs
    c_, rho_ = np.asarray(c_nodal, dtype=np.float64), np.asarray(rho_nodal, dtype=np.float64)
    assert c_.shape == (nd,) and rho_.shape == (nd,)
    Gs, Df = scaled_G(G, 1.0 / rho_, mesh.dofmap), D.flatten()
    cc2 = np.full(nc, -1.0)
    fc1 = (1.0 / rho_)[fd1].mean(axis=1)
    fc2 = -(1.0 / (rho_ * c_))[fd2].mean(axis=1)
    c_ref = float(c_[fd1].mean()) if c_ref is None else float(c_ref)
    w0 = 2 * np.pi * f0
    m = np.zeros(nd)
    oracle_np.mass_apply(np.ones(nd), np.ones(nc), m, detJ, mesh.dofmap)
    m *= 1.0 / (rho_ * c_ * c_)
    term = stage_term(m) if stage_term is not None else None

    def f1(t, ur, un, vn):
        b = np.zeros(nd)
        oracle_np.stiffness_apply(mesh.P, Df, np.ascontiguousarray(ur), cc2, b, Gs, mesh.dofmap)
        if source_term is None:
            T, alpha = 1 / f0, 4.0
            window = 0.5 * (1 - np.cos(f0 * np.pi * t / alpha)) if t < T * alpha else 1.0
            oracle_np.mass_apply(np.full(nd, window * p0 * w0 / c_ref * np.cos(w0 * t)), fc1, b, dF1, fd1)
        else:
            source_term(t, b, (fc1,), dF1, fd1)
        oracle_np.mass_apply(np.ascontiguousarray(vn), fc2, b, dF2, fd2)
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
