"""CPU restatement of the Pennes bioheat solver (bioheat.BioheatSpectral3D) for the tests: the same lumped vectors, the same RK4
sequence and the same dose rule in numpy, fp64, on ``oracle.oracle_np.stiffness_apply`` / ``mass_apply`` with the geometry
``conftest.build_problem`` forms (G, detJ on the host).  Not a test module."""

import numpy as np

from conftest import pkg
from oracle import oracle_np, rk4_oracle

A = (0.0, 0.5, 0.5, 1.0)
B = (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)
C = (0.0, 0.5, 0.5, 1.0)


def rk4_growth(z):
    """rho(z) of classical RK4 for y' = -lambda y, z = lambda dt."""
    return 1.0 - z + z**2 / 2.0 - z**3 / 6.0 + z**4 / 24.0


def gate_of(power):
    if power is None:
        return lambda t: 1.0
    if callable(power):
        return power
    t_on, t_off = power
    return lambda t: 1.0 if t_on <= t < t_off else 0.0


def dose_increment(T, dt):
    """(dt / 60) R^(43 - T), R = 0.5 for T >= 43, 0.25 below."""
    T = np.asarray(T, dtype=np.float64)
    return dt / 60.0 * np.exp2((43.0 - T) * np.where(T >= 43.0, -1.0, -2.0))


def stage_reference(kind, bw, aw, gate, Ta, dt, minv, b, T0, Tn, acc, pr=None, s=None, cem43=None, tmax=None, init=False):
    """One dof-wise stage of csrc/bioheat.hpp in fp64: returns ``(outputs, terms)`` -- the dict of the vectors the kind writes
    and, per output, the sum of the absolute values of the terms it was formed from (what a rounding bound scales with)."""
    f = lambda a: None if a is None else np.asarray(a, dtype=np.float64)  # noqa: E731
    minv, b, T0, Tn, acc, pr, s = (f(a) for a in (minv, b, T0, Tn, acc, pr, s))
    tn = T0 if kind == 0 else Tn
    k, ka = minv * b, np.abs(minv * b)
    if pr is not None:
        k = k - pr * (tn - Ta)
        ka = ka + np.abs(pr * tn) + np.abs(pr * Ta)
    if s is not None:
        k = k + gate * s
        ka = ka + np.abs(gate * s)
    out, terms = {}, {}
    if kind == 2:
        out["T0"], terms["T0"] = acc + bw * k, np.abs(acc) + abs(bw) * ka
        if cem43 is not None:
            inc = dose_increment(out["T0"], dt)
            out["cem43"] = inc if init else f(cem43) + inc
        return out, terms
    base = T0 if kind == 0 else acc
    out["acc"], terms["acc"] = base + bw * k, np.abs(base) + abs(bw) * ka
    out["Tn"], terms["Tn"] = T0 + aw * k, np.abs(T0) + abs(aw) * ka
    return out, terms


class CpuBioheat:
    """M(rho C) dT/dt = -K(k) T - M(w)(T - Ta) + g(t) M(1) q on ``mesh`` (one rank), materials per cell or scalar; ``w`` is the
    product w_b rho_b C_b.  ``fixed``: local dof indices held at their initial value."""

    def __init__(self, mesh, k, rho_c, w=0.0, Ta=37.0, fixed=()):
        self.mesh, self.P, self.Ta = mesh, mesh.P, float(Ta)
        nc = mesh.ncells
        self.G, self.detJ, self.D = rk4_oracle.host_G(mesh), rk4_oracle.host_detJ(mesh), pkg("gll").tabulate_1d(mesh.P, np.float64)[2]
        cell = lambda v: np.full(nc, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)  # noqa: E731
        self.k = cell(k)
        self.mc, self.mw, self.vol = self.lumped(cell(rho_c)), self.lumped(cell(w)), self.lumped(np.ones(nc))
        free = np.ones(mesh.ndofs)
        free[np.asarray(fixed, dtype=np.int64)] = 0.0
        self.free = free
        self.minv = free / self.mc
        self.pr = self.mw * self.minv
        self.s = np.zeros(mesh.ndofs)
        self.T = np.full(mesh.ndofs, 37.0)
        self.cem43, self.tmax = np.zeros(mesh.ndofs), None

    def lumped(self, c):
        y = np.zeros(self.mesh.ndofs)
        oracle_np.mass_apply(np.ones(self.mesh.ndofs), c, y, self.detJ, self.mesh.dofmap)
        return y

    def set_heat_source(self, q):
        self.q = np.asarray(q, dtype=np.float64)
        self.s = self.vol * self.q * self.minv

    def K(self, x):
        """K(k) x."""
        y = np.zeros(self.mesh.ndofs)
        oracle_np.stiffness_apply(self.P, self.D, x, self.k, y, self.G, self.mesh.dofmap)
        return y

    def rhs(self, T, g):
        return -self.minv * self.K(T) - self.pr * (T - self.Ta) + g * self.s

    def advance(self, start_time, final_time, dt, power=None, max_steps=None):
        gate = gate_of(power)
        rk4_steps = pkg("solver_base").rk4_steps
        t, step = float(start_time), 0
        for t0, h in rk4_steps(start_time, final_time, dt, max_steps):
            T0 = self.T
            kk = self.rhs(T0, gate(t0 + C[0] * h))
            acc = T0 + B[0] * h * kk
            for i in (1, 2, 3):
                Tn = T0 + A[i] * h * kk
                kk = self.rhs(Tn, gate(t0 + C[i] * h))
                acc = acc + B[i] * h * kk
            self.T = acc
            self.cem43 = self.cem43 + dose_increment(self.T, h)
            self.tmax = self.T.copy() if self.tmax is None else np.maximum(self.tmax, self.T)
            t, step = t0 + h, step + 1
        return t, step

    def dense_minv_K(self):
        """minv K(k) assembled column by column (small meshes)."""
        n = self.mesh.ndofs
        Kd = np.empty((n, n))
        e = np.zeros(n)
        for j in range(n):
            e[j] = 1.0
            Kd[:, j] = self.K(e)
            e[j] = 0.0
        return self.minv[:, None] * Kd

    def lambda_max(self, iterations=60):
        """A power-iteration estimate of the largest eigenvalue of minv K (a lower bound; for scaling test inputs)."""
        x = np.random.default_rng(5).standard_normal(self.mesh.ndofs) * self.free
        lam = 0.0
        for _ in range(iterations):
            y = self.minv * self.K(x)
            lam = float(x @ (self.mc * y)) / float(x @ (self.mc * x))
            x = y / np.linalg.norm(y)
        return lam


def smooth_field(mesh, seed, modes=3):
    """A smooth random field over the local dofs: a few low Fourier modes with random amplitudes, in [0, 1]."""
    rng = np.random.default_rng(seed)
    X = mesh.dof_coordinates() / np.asarray(getattr(mesh, "length", (1.0, 1.0, 1.0)))
    f = np.zeros(mesh.ndofs)
    for _ in range(modes):
        kx, ky, kz = rng.integers(1, 3, 3)
        f += rng.uniform(0.3, 1.0) * np.cos(np.pi * kx * X[:, 0] + rng.uniform(0, 6)) * np.cos(np.pi * ky * X[:, 1]) * np.cos(np.pi * kz * X[:, 2])
    f -= f.min()
    return f / f.max()
