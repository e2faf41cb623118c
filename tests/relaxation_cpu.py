"""Relaxation mechanisms in the CPU wave model, for the tests: an independent numpy restatement of both solvers with memory variables,

    u' = v,   M v' = r(ur, u, v, t),   xi_nu' = kappa_nu v - xi_nu / tau_nu,        ur = u + sum_nu xi_nu

where the stiffness term of ``r`` acts on ``ur`` and every other term on ``(u, v)``.  The state is larger than the hooks of
``oracle/rk4_oracle.py`` carry, so the classical RK4 loop over ``(u, v, xi)`` is restated here; the operators and the geometry are
the oracle's own (``oracle_np`` / the C restatement, ``rk4_oracle.host_geometry``), unchanged.  Per-cell weights become per-dof ones as
the lumped average ``M(kappa_nu) 1 / M(1) 1``.  With every kappa == 0 the loops reproduce ``rk4_oracle.solve`` / ``solve_westervelt``
bit for bit (tests/test_relaxation.py).  One rank.  Not a test module."""

import numpy as np

from oracle import oracle_np
from oracle.rk4_oracle import A, B, C, host_geometry


def dof_weights(mesh, detJ, kappa, mass):
    """``[NR, ndofs]``: scalar weights broadcast, per-cell weights ``[NR, ncells]`` (the mesh's cell order) as ``M(kappa) 1 / M(1) 1``."""
    kappa = np.asarray(kappa, dtype=np.float64)
    nd = mesh.ndofs
    if kappa.ndim == 1:
        return np.repeat(kappa[:, None], nd, axis=1)
    ones, vol = np.ones(nd), np.zeros(nd)
    mass(ones, np.ones(mesh.ncells), vol, detJ, mesh.dofmap)
    out = np.zeros((kappa.shape[0], nd))
    for nu in range(kappa.shape[0]):
        mass(ones, np.ascontiguousarray(kappa[nu]), out[nu], detJ, mesh.dofmap)
    return out / vol


def rk4_loop(f1, nd, dts, source_time, tau, kd, u=None, v=None, xi=None, record=None):
    """Classical RK4 over ``(u, v, xi)``: ``kv = f1(t, ur, un, vn)``, ``kx = kd vn - xn / tau``.  ``record(t, u, v)`` after every step.
    Returns ``(u, v, xi)``."""
    tau = np.asarray(tau, dtype=np.float64)[:, None]
    u = np.zeros(nd) if u is None else np.array(u, dtype=np.float64)
    v = np.zeros(nd) if v is None else np.array(v, dtype=np.float64)
    xi = np.zeros((tau.shape[0], nd)) if xi is None else np.array(xi, dtype=np.float64)
    ku, kv, kx = np.zeros(nd), np.zeros(nd), np.zeros_like(xi)
    t = 0.0
    for dt in dts:
        u0, v0, x0 = u.copy(), v.copy(), xi.copy()
        for i in range(4):
            un = u0 + A[i] * dt * ku
            vn = v0 + A[i] * dt * kv
            xn = x0 + A[i] * dt * kx
            tn = t + C[i] * dt
            ur = un.copy()
            for row in xn:
                ur = ur + row
            ku = vn.copy()
            kv = f1(tn if source_time == "tn" else t, ur, un, vn)
            kx = kd * vn - xn / tau
            u = u + B[i] * dt * ku
            v = v + B[i] * dt * kv
            xi = xi + B[i] * dt * kx
        t += dt
        if record is not None:
            record(t, u, v)
    return u, v, xi


def _ops(oracle_c, mesh, D, G):
    mass = oracle_c.mass_apply if oracle_c is not None else oracle_np.mass_apply
    if oracle_c is not None:
        stiff = lambda x, cc, y: oracle_c.stiffness_apply(mesh.P, D, x, cc, y, G, mesh.dofmap, threads=1)  # noqa: E731
    else:
        Df = D.flatten()
        stiff = lambda x, cc, y: oracle_np.stiffness_apply(mesh.P, Df, x, cc, y, G, mesh.dofmap)  # noqa: E731
    return mass, stiff


def _window(t, f0):
    T, alpha = 1 / f0, 4.0
    if t < T * alpha:
        return 0.5 * (1 - np.cos(f0 * np.pi * t / alpha)), 0.5 * np.pi * f0 / alpha * np.sin(f0 * np.pi * t / alpha)
    return 1.0, 0.0


def solve(mesh, nsteps, dt, tau, kappa, c0=1500.0, rho0=1000.0, f0=0.5e6, p0=60000.0, source_time="tn", oracle_c=None, c_ref=None,
          u=None, v=None, xi=None, record=None):
    """The linear solver (numba-cpu/demo_linear_box.py:302-455) with mechanisms: ``b = K(-1/rho) ur + facet terms``, ``kv = b / m``.
    ``c0`` / ``rho0``: scalars or per cell; ``kappa``: ``[NR]`` or ``[NR, ncells]``."""
    D, G, detJ, bd1, bd2, dF1, dF2, fd1, fd2 = host_geometry(mesh)
    nc, nd = mesh.ncells, mesh.ndofs
    c_ref = float(c0) if np.ndim(c0) == 0 else (float(np.asarray(c0)[bd1[:, 0]].mean()) if c_ref is None else float(c_ref))
    c_, rho_ = (np.broadcast_to(np.asarray(a, dtype=np.float64), (nc,)).copy() for a in (c0, rho0))
    cc1, cc2 = 1 / rho_ / c_ / c_, -1 / rho_
    fc1, fc2 = 1 / rho_[bd1[:, 0]], -1 / rho_[bd2[:, 0]] / c_[bd2[:, 0]]
    w0 = 2 * np.pi * f0
    mass, stiff = _ops(oracle_c, mesh, D, G)
    m = np.zeros(nd)
    mass(np.ones(nd), cc1, m, detJ, mesh.dofmap)
    kd = dof_weights(mesh, detJ, kappa, mass)

    def f1(t, ur, un, vn):
        b = np.zeros(nd)
        stiff(np.ascontiguousarray(ur), cc2, b)
        mass(np.full(nd, _window(t, f0)[0] * p0 * w0 / c_ref * np.cos(w0 * t)), fc1, b, dF1, fd1)
        mass(np.ascontiguousarray(vn), fc2, b, dF2, fd2)
        return b / m

    dts = list(dt) if hasattr(dt, "__len__") else [dt] * nsteps
    return rk4_loop(f1, nd, dts, source_time, tau, kd, u, v, xi, record)


def solve_westervelt(mesh, nsteps, dt, tau, kappa, c0=1480.0, rho0=1000.0, f0=1.1e6, p0=None, beta=3.5, att_dB=0.2, source_time="tn",
                     oracle_c=None, u=None, v=None, xi=None, record=None):
    """The Westervelt solver (cuda/demo_nonlinear_bowl.py:357-374,458-475,540-650) with mechanisms: ``K(c3) ur + K(c4) vn``; the
    lumped mass ``m0 + M(c2) un``, the quadratic term and the facet terms see ``(un, vn)``."""
    D, G, detJ, bd1, bd2, dF1, dF2, fd1, fd2 = host_geometry(mesh)
    nc, nd = mesh.ncells, mesh.ndofs
    c_ref = float(c0) if np.ndim(c0) == 0 else float(np.asarray(c0)[bd1[:, 0]].mean())
    rho_ref = float(rho0) if np.ndim(rho0) == 0 else float(np.asarray(rho0)[bd1[:, 0]].mean())
    if p0 is None:
        p0 = rho_ref * c_ref * 0.38557513826589934
    w0 = 2 * np.pi * f0
    c_, rho_, beta_, att_ = (np.broadcast_to(np.asarray(a, dtype=np.float64), (nc,)).copy() for a in (c0, rho0, beta, att_dB))
    delta = 2 * (att_ / 20 * np.log(10)) * c_**3 / w0 / w0
    cc1, cc2, cc3 = 1 / rho_ / c_**2, -2 * beta_ / rho_**2 / c_**4, -1 / rho_
    cc4, cc5 = -delta / rho_ / c_**2, 2 * beta_ / rho_**2 / c_**4
    i1, i2 = bd1[:, 0], bd2[:, 0]
    f11, f21 = 1 / rho_[i1], delta[i1] / rho_[i1] / c_[i1] ** 2
    f12, f22 = delta[i2] / rho_[i2] / c_[i2] ** 3, -1 / rho_[i2] / c_[i2]
    _, stiff = _ops(oracle_c, mesh, D, G)
    mass = oracle_np.mass_apply
    ones, m0 = np.ones(nd), np.zeros(nd)
    mass(ones, cc1, m0, detJ, mesh.dofmap)
    mass(ones, f12, m0, dF2, fd2)
    kd = dof_weights(mesh, detJ, kappa, mass)
    a = 2 * p0 * w0 / c_ref

    def f1(t, ur, un, vn):
        m = np.zeros(nd)
        mass(np.ascontiguousarray(un), cc2, m, detJ, mesh.dofmap)
        m += m0
        b = np.zeros(nd)
        stiff(np.ascontiguousarray(ur), cc3, b)
        stiff(np.ascontiguousarray(vn), cc4, b)
        mass(vn * vn, cc5, b, detJ, mesh.dofmap)
        window, dwindow = _window(t, f0)
        mass(np.full(nd, window * a * np.cos(w0 * t)), f11, b, dF1, fd1)
        mass(np.full(nd, dwindow * a * np.cos(w0 * t) - window * a * w0 * np.sin(w0 * t)), f21, b, dF1, fd1)
        mass(np.ascontiguousarray(vn), f22, b, dF2, fd2)
        return b / m

    dts = list(dt) if hasattr(dt, "__len__") else [dt] * nsteps
    return rk4_loop(f1, nd, dts, source_time, tau, kd, u, v, xi, record)


# ---- the plane-wave absorption experiment, shared by the CPU and the GPU test ------------------------------------------------------
def plane_wave_case():
    """A row of cubic cells one cell wide (rigid lateral walls: the plane wave is exact), about 20 wavelengths long, continuous wave,
    homogeneous weights chosen so that the amplitude falls by more than e^-0.5 over the fitted stretch."""
    import fusgpu_loader

    boxmesh, ls, rx = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "relaxation"))
    P, c, f0, nx = 4, 1500.0, 0.5e6, 60
    lam = c / f0
    L, h = 20 * lam, 20 * lam / nx
    mesh = boxmesh.BoxMesh(P, (nx, 1, 1), length=(L, h, h))
    hmin = ls.time_step_parameters(mesh, P, c, f0, L)
    dt, _, _ = ls.snap_time_step(hmin, P, c, f0, L)
    per = int(round(1.0 / f0 / dt))
    # the weights of a 2-mechanism fit of 0.5 dB/cm/MHz^1.1 between 0.25 and 2.5 MHz, scaled up so that alpha_r (w0) 18 lambda = 0.6
    fit = rx.fit_power_law(0.5, 1.1, 0.25e6, 2.5e6, n=2, speed_of_sound=c, with_thermoviscous=False)
    model = rx.RelaxationAbsorption(fit.tau, fit.kappa)
    model = rx.RelaxationAbsorption(fit.tau, fit.kappa * (0.6 / (18 * lam)) / model.alpha(f0, c))
    return dict(mesh=mesh, P=P, c=c, f0=f0, lam=lam, L=L, dt=dt, per=per, periods=30, model=model, x_fit=(1.0 * lam, 19.0 * lam))


def fit_slopes(x, amplitude, phase, lo, hi):
    """Least-squares slopes of ``log amplitude`` and of the unwrapped ``phase`` against ``x`` over ``lo <= x <= hi``:
    ``(alpha, k)`` of a wave ``A e^{-alpha x} cos(w t - k x)``."""
    order = np.argsort(x, kind="stable")
    x, amplitude, phase = x[order], amplitude[order], phase[order]
    ph = np.unwrap(phase)
    keep = (x >= lo) & (x <= hi)
    alpha = -np.polyfit(x[keep], np.log(amplitude[keep]), 1)[0]
    k = -np.polyfit(x[keep], ph[keep], 1)[0]
    return float(alpha), float(k)
