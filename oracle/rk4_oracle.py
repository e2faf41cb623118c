"""ORACLE-side wave model (test infrastructure -- NOT product code): the linear wave solver of
numba-cpu/demo_linear_box.py:302-455 (f0 / f1 / RK4 loop, source evaluated at tn) and the Westervelt
solver of cuda/demo_nonlinear_bowl.py:357-374,458-475,540-650 on one rank, restated with the oracle's
operators.  Pinned against the reference-driven fixtures tests/golden/rk4_*.npz / rk4nl_*.npz
(tests/test_rk4_golden.py).  Used to check the GPU solvers' pressure fields -- in tests/ and as the CHECKER of every RK4 /
Westervelt step line of bench.py (benchlib/cpu_legs.py oracle_step_field) -- and by bench.py's ``cpu_baseline`` leg of the RK4-step line
(the reference prints "Solve time per step" of exactly this loop, numba-cpu/demo_linear_box.py:472-473).

One model: ``host_geometry`` (with its parts ``host_G`` / ``host_detJ`` / ``host_facet_detJ``) is the one place that forms the host geometry factors,
``rk4_loop`` the one time loop; ``solve`` and ``solve_westervelt`` each add their coefficients and their right-hand side ``f1``.  What
a feature adds to a stage enters through two hooks instead of a copy of the loop: ``stage_term`` (the sponge layer of
tests/sponge_cpu.py) and ``source_term`` (the per-element array source of tests/test_sources_gpu.py).  Absent, a hook costs a stage
nothing: the array operations are those of the reference's loop.

Only tests/, __graft_entry__.smoke() and bench.py's checker / cpu_baseline legs (benchlib/) import this: never the product.  The mesh / table builders
it takes from the package (gll, precompute: host-side numpy, the counterparts of what the reference takes from
basix / dolfinx) are inputs, not the operators under test."""

import time
from collections import namedtuple

import numpy as np

import fusgpu_loader
from oracle import oracle_np


def pkg(name):
    return fusgpu_loader.submodule(name)


A = (0.0, 0.5, 0.5, 1.0)
B = (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)
C = (0.0, 0.5, 0.5, 1.0)


def step_sizes(t0, tf, dt):
    """The reference's time loop (``while t < tf: dt = min(dt, tf - t); ...; t += dt``,
    cuda/demo_linear_box.py:487-488,566): the last step may be shorter."""
    out, t = [], float(t0)
    while t < tf:
        dt = min(dt, tf - t)
        out.append(dt)
        t += dt
    return out


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
HostGeometry = namedtuple("HostGeometry", "D G detJ bd1 bd2 dF1 dF2 fd1 fd2")
"""``D``: the 1-D derivative table; ``G``, ``detJ``: the cells' scaled geometry factors; ``bd1`` / ``bd2``: the (cell, local facet) rows of
the facets tagged 2 (source) / 3 (absorbing), ``dF1`` / ``dF2`` their scaled ``detJ``, ``fd1`` / ``fd2`` their facet dofmaps."""


def _cell_tables(P):
    """The trilinear geometry gradients at the cell's GLL points and the points' weights."""
    gll = pkg("gll")
    pts, wts, _ = gll.tabulate_1d(P)
    return pkg("precompute").tabulate_hex_p1_gradients(gll.tensor_points_3d(pts)), gll.tensor_weights_3d(wts)


def host_G(mesh):
    """``G[ncells, n^3, 6]`` of ``mesh`` (every cell of the rank), on the host in fp64."""
    G = np.zeros((mesh.ncells, (mesh.P + 1) ** 3, 6))
    pkg("precompute").compute_scaled_geometrical_factor(G, (mesh.x_dofs, mesh.x_g), mesh.ncells, *_cell_tables(mesh.P))
    return G


def host_detJ(mesh):
    """``detJ[ncells, n^3]`` of ``mesh``, on the host in fp64."""
    detJ = np.zeros((mesh.ncells, (mesh.P + 1) ** 3))
    pkg("precompute").compute_scaled_jacobian_determinant(detJ, (mesh.x_dofs, mesh.x_g), mesh.ncells, *_cell_tables(mesh.P))
    return detJ


def host_facet_detJ(mesh, bd):
    """``detJ_f[nfacets, n^2]`` of the boundary facets ``bd`` (rows of (cell, local facet)), on the host in fp64."""
    gll, pre = pkg("gll"), pkg("precompute")
    pts, wts, _ = gll.tabulate_1d(mesh.P)
    dF = np.zeros((bd.shape[0], (mesh.P + 1) ** 2))
    pre.compute_boundary_facets_scaled_jacobian_determinant(dF, (mesh.x_dofs, mesh.x_g), bd, pre.tabulate_facet_gradients(pts), gll.tensor_weights_2d(wts))
    return dF


def host_geometry(mesh, factors=None):
    """Everything geometric the two solvers read, on the host in fp64, as a ``HostGeometry``.  ``factors = (G, detJ, dF1, dF2)``: those
    arrays are used as they are and the host precompute is skipped."""
    D = pkg("gll").tabulate_1d(mesh.P)[2]
    bd1, bd2 = mesh.boundary_facets([2]), mesh.boundary_facets([3])
    if factors is not None:
        G, detJ, dF1, dF2 = factors
    else:
        G, detJ, dF1, dF2 = host_G(mesh), host_detJ(mesh), host_facet_detJ(mesh, bd1), host_facet_detJ(mesh, bd2)
    return HostGeometry(D, G, detJ, bd1, bd2, dF1, dF2, mesh.facet_dofmap(bd1), mesh.facet_dofmap(bd2))


# ---- the time loop -----------------------------------------------------------------------------------------------------------------
def rk4_loop(f1, nd, dts, source_time, u=None, v=None, timing=None):
    """The reference's RK4 loop over the step sizes ``dts`` from the state ``(u, v)`` (zero when absent): ``kv = f1(t, un, vn)`` with the
    stage time ``tn`` or, ``source_time == "t"``, the step's start.  ``timing``: a dict that receives ``seconds_per_step`` (this loop
    alone) and ``steps``."""
    u = np.zeros(nd) if u is None else np.array(u, dtype=np.float64)
    v = np.zeros(nd) if v is None else np.array(v, dtype=np.float64)
    ku, kv = np.zeros(nd), np.zeros(nd)
    t = 0.0
    t_loop = time.perf_counter()
    for dt in dts:
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
    if timing is not None:
        timing["seconds_per_step"] = (time.perf_counter() - t_loop) / max(len(dts), 1)
        timing["steps"] = len(dts)
    return u, v


def _dts(nsteps, dt):
    return list(dt) if hasattr(dt, "__len__") else [dt] * nsteps


def _stiffness(mesh, D, G, oracle_c, threads):
    """``stiff(x, cc, y)``: y += K(cc) x with the C restatement of the operator (``threads`` > 1: its OpenMP apply) or the numpy one."""
    if oracle_c is not None:
        return lambda x, cc, y: oracle_c.stiffness_apply(mesh.P, D, x, cc, y, G, mesh.dofmap, threads=threads)
    Df = D.flatten()
    return lambda x, cc, y: oracle_np.stiffness_apply(mesh.P, Df, x, cc, y, G, mesh.dofmap)


# ---- the two solvers ---------------------------------------------------------------------------------------------------------------
# Common keyword arguments.  ``u``, ``v``: the initial state.  ``facets=False`` drops every boundary-facet term.  ``stage_term(m)``, called
# once with the complete lumped mass, returns ``term(b, un, vn)``, applied to a stage's right-hand side just before ``b / m``.
# ``source_term(t, b, coefficients, detJ, dofmap)`` adds the source facets' part of a stage at the source time ``t`` in place of the
# model's uniform source: it gets the source set's per-facet coefficient(s), scaled detJ and dofmap (the absorbing set stays here).
def solve(mesh, nsteps, dt, c0=1500.0, rho0=1000.0, f0=0.5e6, p0=60000.0, source_time="tn", oracle_c=None, threads=1, timing=None,
          geometry=None, c_ref=None, u=None, v=None, facets=True, stage_term=None, source_term=None):
    """``dt`` may be a sequence of per-step sizes (then ``nsteps`` is ignored).  ``oracle_c``: the C restatement of the
    operators instead of the numpy one (``threads`` > 1: its OpenMP stiffness apply).  ``timing``: a dict that receives
    ``seconds_per_step`` (the time loop alone, set-up excluded -- what the reference prints as "Solve time per step").
    ``geometry = (G, detJ, detJ_f1, detJ_f2)``: geometry factors computed elsewhere (bench.py hands over the ones the GPU
    stepped with) instead of the host precompute."""
    D, G, detJ, bd1, bd2, dF1, dF2, fd1, fd2 = host_geometry(mesh, geometry)
    nc, nd = mesh.ncells, mesh.ndofs
    # c0 / rho0: scalars or one value per cell (heterogeneous medium); the source term uses the scalar ``c_ref``
    c_ref = float(c0) if np.ndim(c0) == 0 else (float(np.asarray(c0)[bd1[:, 0]].mean()) if c_ref is None else float(c_ref))
    c_, rho_ = (np.broadcast_to(np.asarray(a, dtype=np.float64), (nc,)).copy() for a in (c0, rho0))
    cc1, cc2 = 1 / rho_ / c_ / c_, -1 / rho_
    fc1, fc2 = 1 / rho_[bd1[:, 0]], -1 / rho_[bd2[:, 0]] / c_[bd2[:, 0]]
    c0 = c_ref
    w0 = 2 * np.pi * f0
    m = np.zeros(nd)
    mass = oracle_c.mass_apply if oracle_c is not None else oracle_np.mass_apply
    mass(np.ones(nd), cc1, m, detJ, mesh.dofmap)
    stiff = _stiffness(mesh, D, G, oracle_c, threads)
    term = stage_term(m) if stage_term is not None else None

    def f1(t, un, vn):
        b = np.zeros(nd)
        stiff(un, cc2, b)
        if facets:
            if source_term is None:
                T, alpha = 1 / f0, 4.0
                window = 0.5 * (1 - np.cos(f0 * np.pi * t / alpha)) if t < T * alpha else 1.0
                mass(np.full(nd, window * p0 * w0 / c0 * np.cos(w0 * t)), fc1, b, dF1, fd1)
            else:
                source_term(t, b, (fc1,), dF1, fd1)
            mass(np.ascontiguousarray(vn), fc2, b, dF2, fd2)
        if term is not None:
            term(b, un, vn)
        return b / m

    return rk4_loop(f1, nd, _dts(nsteps, dt), source_time, u, v, timing)


def solve_westervelt(mesh, nsteps, dt, c0=1480.0, rho0=1000.0, f0=1.1e6, p0=None, beta=3.5, att_dB=0.2,
                     source_time="tn", oracle_c=None, c_ref=None, rho_ref=None, threads=1, geometry=None, u=None, v=None, facets=True,
                     stage_term=None, source_term=None, timing=None):
    """cuda/demo_nonlinear_bowl.py:357-374,458-475,540-650 restated with the oracle's operators
    (single rank; source on x = 0, absorbing on x = L).  ``oracle_c``: the C restatement of the operators (``threads`` > 1: its
    OpenMP stiffness apply).  ``geometry = (G, detJ, detJ_f1, detJ_f2)``: geometry factors computed elsewhere (bench.py hands
    over the ones the GPU stepped with) instead of the host precompute.  ``stage_term`` is called with the steady lumped mass m0;
    ``source_term`` gets the coefficients of the source and of its time derivative."""
    D, G, detJ, bd1, bd2, dF1, dF2, fd1, fd2 = host_geometry(mesh, geometry)
    # c0, rho0, beta, att_dB: scalars or one value per cell; the source term and the default amplitude use scalars (c_ref, rho_ref)
    c_ref = float(c0) if np.ndim(c0) == 0 else (float(np.asarray(c0)[bd1[:, 0]].mean()) if c_ref is None else float(c_ref))
    rho_ref = float(rho0) if np.ndim(rho0) == 0 else (float(np.asarray(rho0)[bd1[:, 0]].mean()) if rho_ref is None else float(rho_ref))
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
    c0 = c_ref  # from here on: the scalar of the source term
    nd = mesh.ndofs
    ones = np.ones(nd)
    m0 = np.zeros(nd)
    # the mass applies: the numpy restatement, or (large meshes) the C one -- both pinned by tests/test_oracle_golden.py
    mass_apply = oracle_c.mass_apply if (oracle_c is not None and geometry is not None) else oracle_np.mass_apply
    oracle_np.mass_apply(ones, cc1, m0, detJ, mesh.dofmap)
    if facets:
        oracle_np.mass_apply(ones, f12, m0, dF2, fd2)
    stiff = _stiffness(mesh, D, G, oracle_c, threads)
    term = stage_term(m0) if stage_term is not None else None

    def f1(t, un, vn):
        m = np.zeros(nd)
        mass_apply(np.ascontiguousarray(un), cc2, m, detJ, mesh.dofmap)
        m += m0
        b = np.zeros(nd)
        stiff(np.ascontiguousarray(un), cc3, b)
        stiff(np.ascontiguousarray(vn), cc4, b)
        mass_apply(vn * vn, cc5, b, detJ, mesh.dofmap)
        if facets:
            if source_term is None:
                T, alpha = 1 / f0, 4.0
                if t < T * alpha:
                    window = 0.5 * (1 - np.cos(f0 * np.pi * t / alpha))
                    dwindow = 0.5 * np.pi * f0 / alpha * np.sin(f0 * np.pi * t / alpha)
                else:
                    window, dwindow = 1.0, 0.0
                a = 2 * p0 * w0 / c0
                mass_apply(np.full(nd, window * a * np.cos(w0 * t)), f11, b, dF1, fd1)
                mass_apply(np.full(nd, dwindow * a * np.cos(w0 * t) - window * a * w0 * np.sin(w0 * t)), f21, b, dF1, fd1)
            else:
                source_term(t, b, (f11, f21), dF1, fd1)
            mass_apply(np.ascontiguousarray(vn), f22, b, dF2, fd2)
        if term is not None:
            term(b, un, vn)
        return b / m

    return rk4_loop(f1, nd, _dts(nsteps, dt), source_time, u, v, timing)
