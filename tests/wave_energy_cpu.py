"""Energy and step bound of the two wave solvers in the CPU wave model (``oracle/rk4_oracle.py``), for the tests: on tiny meshes the
lumped mass, the DENSE stiffness (the oracle's apply on unit vectors), the absorbing-facet and sponge diagonals and the dense
first-order matrix of the linear(ised) system

    u' = v,    M v' = -(K + S2 M) u - (C + F + 2 S M) v        K = K(1/rho),  C = K(delta / (rho c^2)) (Westervelt),
                                                                F = diag(M_f2(1/(rho c)) 1),  S = diag(sigma)

whose spectrum gives the TRUE RK4 limit ``dt*`` (the largest dt with max_j |R(dt mu_j)| <= 1) that ``stable_time_step`` is held
against, the conserved form ``E = 1/2 v.M v + 1/2 u.K u`` and the time loop of the same runs.  One rank.  Not a test module."""
import functools

import numpy as np

import sponge_cpu
from conftest import pkg
from oracle import oracle_np, rk4_oracle

LENGTH = 0.01
F0 = 0.5e6


def box(P=2, cells=(3, 2, 2), perturb=0.15, seed=3, grid=(1, 1, 1), rank=0, dtype=np.float64):
    return pkg("boxmesh").BoxMesh(P, cells, grid=grid, rank=rank, length=LENGTH, perturb=perturb, seed=seed, dtype=dtype)


def centroids(mesh):
    return np.asarray(mesh.x_g, dtype=np.float64)[mesh.x_dofs].mean(axis=1)


def two_materials(mesh):
    """Water in the half of the box next to the source, bone beyond: ``(c, rho)`` per cell, decided by the cell's centroid so that
    every partition of the box sees the same medium."""
    bone = centroids(mesh)[:, 0] > 0.5 * LENGTH
    return np.where(bone, 2800.0, 1500.0), np.where(bone, 1850.0, 1000.0)


def sponge_profile(sigma_max):
    """sigma(xyz): a quadratic ramp over the last 40 % of the box along y (away from the source and absorbing faces)."""
    def sigma(xyz):
        depth = np.clip((np.asarray(xyz)[:, 1] / LENGTH - 0.6) / 0.4, 0.0, 1.0)
        return sigma_max * depth**2

    return sigma


def attenuation_for(ratio_times_root, c, lam, f0=F0):
    """The attenuation in dB/m at which ``delta / c^2 * sqrt(lam) = ratio_times_root`` for the speed ``c``: delta = 2 a c^3 / w0^2."""
    w0 = 2.0 * np.pi * f0
    return ratio_times_root / np.sqrt(lam) * w0 * w0 / (2.0 * c) * 20.0 / np.log(10.0)


class Dense:
    """The dense operators of one configuration on ``mesh``.  ``kind``: ``"linear"`` or ``"westervelt"``; ``c``, ``rho``, ``att_dB``:
    per cell; ``sigma``: None or a callable of the dof coordinates.  ``nodal = (c, rho)`` at the dofs (linear): the lumped mass is
    ``M(1) 1 / (rho c^2)``, the stiffness carries ``1/rho`` in its geometric factor (tests/nodal_cpu.py) and the absorbing facets one
    mean of ``1/(rho c)`` each; ``c`` and ``rho`` are then the per-cell means."""

    def __init__(self, mesh, kind, c, rho, sigma=None, att_dB=0.0, f0=F0, nodal=None):
        self.mesh, self.kind, self.f0 = mesh, kind, f0
        geo = rk4_oracle.host_geometry(mesh)
        nd, nc = mesh.ndofs, mesh.ncells
        self.c, self.rho = (np.broadcast_to(np.asarray(a, dtype=np.float64), (nc,)).copy() for a in (c, rho))
        self.att_dB = np.broadcast_to(np.asarray(att_dB, dtype=np.float64), (nc,)).copy()
        w0 = 2.0 * np.pi * f0
        self.delta = 2.0 * (self.att_dB / 20.0 * np.log(10.0)) * self.c**3 / w0 / w0 if kind == "westervelt" else np.zeros(nc)
        ones = np.ones(nd)
        self.m = np.zeros(nd)
        oracle_np.mass_apply(ones, 1.0 / self.rho / self.c**2, self.m, geo.detJ, mesh.dofmap)
        i2 = geo.bd2[:, 0]
        if kind == "westervelt":  # the steady lumped mass m0 carries the absorbing facets' delta / (rho c^3)
            oracle_np.mass_apply(ones, self.delta[i2] / self.rho[i2] / self.c[i2] ** 3, self.m, geo.dF2, geo.fd2)
        self.facet = np.zeros(nd)
        oracle_np.mass_apply(ones, 1.0 / self.rho[i2] / self.c[i2], self.facet, geo.dF2, geo.fd2)
        self.K = self._dense(geo, 1.0 / self.rho)
        if nodal is not None:
            c_n, rho_n = (np.asarray(a, dtype=np.float64) for a in nodal)
            self.m = np.zeros(nd)
            oracle_np.mass_apply(ones, np.ones(nc), self.m, geo.detJ, mesh.dofmap)
            self.m /= rho_n * c_n**2
            self.facet = np.zeros(nd)
            oracle_np.mass_apply(ones, (1.0 / (rho_n * c_n))[geo.fd2].mean(axis=1), self.facet, geo.dF2, geo.fd2)
            self.K = self._dense(geo._replace(G=geo.G * (1.0 / rho_n)[mesh.dofmap][:, :, None]), np.ones(nc))
        self.C = self._dense(geo, self.delta / self.rho / self.c**2) if kind == "westervelt" else np.zeros((nd, nd))
        self.sigma_fn = sigma
        self.sigma = np.zeros(nd) if sigma is None else np.asarray(sigma(mesh.dof_coordinates()), dtype=np.float64)

    def _dense(self, geo, cc):
        nd, Df = self.mesh.ndofs, geo.D.flatten()
        A = np.zeros((nd, nd))
        for j in range(nd):
            e = np.zeros(nd)
            e[j] = 1.0
            oracle_np.stiffness_apply(self.mesh.P, Df, e, cc, A[:, j], geo.G, self.mesh.dofmap)
        return 0.5 * (A + A.T)

    # -- the two bounds at exact eigenvalues, and the true limit -------------------------------------------------------------------
    def lambda_max(self):
        s = 1.0 / np.sqrt(self.m)
        return float(np.linalg.eigvalsh(s[:, None] * self.K * s[None, :])[-1])

    def damping_max(self):
        return float(np.max(self.facet / self.m + 2.0 * self.sigma)) + float(np.max(self.delta / self.c**2)) * self.lambda_max()

    def formula(self, safety=1.0):
        """``stable_time_step(safety)`` at exact eigenvalues."""
        return safety * pkg("stability").rk4_stable_step(self.lambda_max() + float(np.max(self.sigma**2)), self.damping_max())

    def first_order_matrix(self):
        nd, minv = self.mesh.ndofs, 1.0 / self.m
        A = np.zeros((2 * nd, 2 * nd))
        A[:nd, nd:] = np.eye(nd)
        A[nd:, :nd] = -(minv[:, None] * self.K) - np.diag(self.sigma**2)
        A[nd:, nd:] = -(minv[:, None] * self.C) - np.diag(minv * self.facet + 2.0 * self.sigma)
        return A

    def true_limit(self):
        """dt*: the first dt at which some eigenvalue of the first-order matrix leaves RK4's stability region (scan, then bisection)."""
        st = pkg("stability")
        mu = np.linalg.eigvals(self.first_order_matrix())
        mu = mu[np.abs(mu) > 1e-9 * np.abs(mu).max()]  # the constant mode: R(0) = 1
        slack = 1.0 + 1e-9  # (a defective or nearly repeated eigenvalue is computed to ~sqrt(eps))
        grid = 8.0 / np.abs(mu).max() * np.arange(1, 8193) / 8192
        ok = np.array([np.all(st.rk4_growth(mu * dt) <= slack) for dt in grid])
        first = int(np.argmin(ok))
        lo, hi = (grid[first - 1] if first else 0.0), grid[first]
        for _ in range(100):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if np.all(st.rk4_growth(mu * mid) <= slack) else (lo, mid)
        return float(lo)

    # -- the conserved form and the time loop ---------------------------------------------------------------------------------------
    def energy(self, u, v):
        """``(kinetic, potential)`` of the state."""
        u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        return 0.5 * float(v @ (self.m * v)), 0.5 * float(u @ (self.K @ u))

    def run(self, u, v, nsteps, dt):
        """The states after each of ``nsteps`` steps of the CPU model from ``(u, v)``, source off: ``[(u_1, v_1), ...]``."""
        term = None if self.sigma_fn is None else sponge_cpu.layer_term(self.mesh, self.sigma_fn)
        states = []
        for _ in range(nsteps):
            if self.kind == "linear":
                u, v = rk4_oracle.solve(self.mesh, 1, dt, c0=self.c, rho0=self.rho, f0=self.f0, p0=0.0, u=u, v=v, stage_term=term)
            else:
                u, v = rk4_oracle.solve_westervelt(self.mesh, 1, dt, c0=self.c, rho0=self.rho, f0=self.f0, p0=0.0, att_dB=self.att_dB,
                                                   u=u, v=v, stage_term=term)
            states.append((u, v))
        return states


def pulse(mesh, amplitude=1.0, width=0.12, center=(0.5, 0.5, 0.5)):
    """A Gaussian of ``amplitude`` at ``center`` (fractions of the box), ``width`` of the box wide: negligible at the faces."""
    r2 = np.sum((np.asarray(mesh.dof_coordinates(), dtype=np.float64) / LENGTH - np.asarray(center)) ** 2, axis=1)
    return amplitude * np.exp(-r2 / (width * width))


def smooth_state(mesh, seed=0):
    """A seeded smooth ``(u, v)``: a few low Fourier modes with random coefficients; v of the size c k u."""
    rng = np.random.default_rng(seed)
    x = np.asarray(mesh.dof_coordinates(), dtype=np.float64) / LENGTH
    u, v = np.zeros(mesh.ndofs), np.zeros(mesh.ndofs)
    for _ in range(4):
        k, ph = rng.integers(1, 3, size=3), rng.uniform(0, 2 * np.pi, size=2)
        u += rng.uniform(0.5, 1.0) * np.sin(np.pi * (x @ k) + ph[0])
        v += rng.uniform(0.5, 1.0) * np.cos(np.pi * (x @ k) + ph[1]) * 1500.0 * np.pi / LENGTH
    return u, v


@functools.lru_cache(maxsize=None)
def configuration(name):
    """The three dense configurations of the step bound, each P = 2 on (3, 2, 2) perturbed cells: ``linear`` (two materials),
    ``sponge`` (linear, a layer whose sigma_max = 1.5 sqrt(lambda_max) makes the damping the binding term: 2.785 / (2 sigma_max)
    is a third of 2 sqrt 2 / sqrt(lambda_max)), ``westervelt`` (an attenuation at which max(delta / c^2) sqrt(lambda_max) = 0.8:
    the diffusivity's damping rate is of the size of the largest frequency)."""
    mesh = box()
    c, rho = two_materials(mesh)
    if name == "linear":
        return Dense(mesh, "linear", c, rho)
    lam = Dense(mesh, "linear", c, rho).lambda_max()
    if name == "sponge":
        return Dense(mesh, "linear", c, rho, sigma=sponge_profile(1.5 * np.sqrt(lam)))
    if name == "westervelt":
        return Dense(mesh, "westervelt", c, rho, att_dB=attenuation_for(0.8, c.max(), lam) * np.ones(mesh.ncells))
    raise KeyError(name)
