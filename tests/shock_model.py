"""The shock-capturing sensor (csrc/modal_sensor.hpp, include/fus_gpu_sensor.h) as plain fp64 numpy, with a running error bound of
its two energies, and the CPU model of a run with it: the oracle's Westervelt loop (``oracle/rk4_oracle.py``) with the extra stage term
``K(-eps scale) v_n`` through its ``stage_term`` hook, stepped in segments of ``every`` steps with this sensor between them.  One rank.
Not a test module.

The bound follows the kernel's operation sequence, not what the device returns.  With ``n = P + 1``, ``u_T`` the unit round-off of the
field type and ``A = (|Vinv| x |Vinv| x |Vinv|) |u|`` (the same transform on absolute values):

  transform   three passes, each a dot product of n terms in the field type: at most 2 n roundings per pass (n with fused
              multiply-add), so a computed mode differs from the exact one by at most d = ((1 + u_T)^(6 n) - 1) A <= 6 n u_T A (1 + ...)
  squares     (m + d)^2 - m^2 <= 2 |m| d + d^2 <= (2 c + c^2) A^2 with c = 6 n u_T (1 + 6 n u_T), because |m| <= A
  sums        in double: a product, then at most n - 1 additions in the thread, n - 1 over the row, n - 1 over the rows: every term
              passes through at most 3 n roundings, each relative to a partial sum of non-negative terms <= sum A^2
  the model   forms the same transform in double: the same expression with u_T = 2^-53 once more

so ``|E_device - E_model| <= [(2 c + c^2) + c_64 (2 + c_64) + 3 n 2^-53] sum_k A_k^2`` over the modes ``k`` of the energy (all of them
for ``tot``, the shell for ``top``).  The comparison of ``top`` is ABSOLUTE against this bound: for a smooth field ``top`` is what the
cancellation in the transform leaves, and a relative tolerance would be meaningless."""
import functools

import numpy as np
from numpy.polynomial import legendre as leg

from conftest import pkg
from oracle import oracle_np, rk4_oracle

QUIET = -1000.0  # FUS_SENSOR_QUIET (tests/test_shock_capture.py holds it against the header)
U64, U32 = 2.0**-53, 2.0**-24


def unit_roundoff(dtype):
    return U64 if np.dtype(dtype) == np.float64 else U32


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def vandermonde(P):
    """V[j][k] = sqrt((2k + 1) / 2) P_k(xi_j) at the nodes in the order ``gll.tabulate_1d(P)`` returns them, by ``legval``."""
    xi = 2.0 * np.asarray(pkg("gll").tabulate_1d(P)[0], dtype=np.float64) - 1.0
    V = np.zeros((P + 1, P + 1))
    for k in range(P + 1):
        c = np.zeros(k + 1)
        c[k] = np.sqrt((2 * k + 1) / 2.0)
        V[:, k] = leg.legval(xi, c)
    return V


def table(P, dtype=np.float64):
    """Vinv [mode, node] as the kernel reads it: the fp64 inverse rounded to ``dtype``, returned in fp64."""
    return np.linalg.inv(vandermonde(P)).astype(dtype).astype(np.float64)


# ---- the sensor ----------------------------------------------------------------------------------------------------------------------
def transform(Vinv, ue):
    """``ue`` [ncell, n, n, n] (tx, ty, tz) -> modes [ncell, kx, ky, kz]."""
    return np.einsum("ai,bj,ck,eijk->eabc", Vinv, Vinv, Vinv, ue, optimize=True)


def shell(P):
    k = np.arange(P + 1)
    return (k[:, None, None] == P) | (k[None, :, None] == P) | (k[None, None, :] == P)


def energies(Vinv, u, dofmap, P, dtype=np.float64):
    """``(tot, top, bound_tot, bound_top)`` per cell of the field ``u`` (values as the device holds them, any float type)."""
    n = P + 1
    ue = np.asarray(u, dtype=np.float64)[np.asarray(dofmap)].reshape(-1, n, n, n)
    m = transform(Vinv, ue)
    A2 = transform(np.abs(Vinv), np.abs(ue)) ** 2
    sh = shell(P)
    ut = unit_roundoff(dtype)
    c, c64 = 6 * n * ut * (1 + 6 * n * ut), 6 * n * U64 * (1 + 6 * n * U64)
    k = (2 * c + c * c) + c64 * (2 + c64) + 3 * n * U64
    m2 = m * m
    return m2.sum(axis=(1, 2, 3)), m2[:, sh].sum(axis=1), k * A2.sum(axis=(1, 2, 3)), k * A2[:, sh].sum(axis=1)


def ramp(s, s0, kappa):
    s = np.asarray(s, dtype=np.float64)
    mid = 0.5 * (1.0 + np.sin(0.5 * np.pi * np.clip((s - s0) / kappa, -1.0, 1.0)))
    return np.where(s <= s0 - kappa, 0.0, np.where(s >= s0 + kappa, 1.0, mid))


def sense(tot, top, floor, s0, kappa):
    """``(s, r)`` per cell: the sentinel and 0 where the cell is quiet or ``top`` is not positive."""
    tot, top = np.asarray(tot, dtype=np.float64), np.asarray(top, dtype=np.float64)
    loud = ~(tot <= 8.0 * floor * floor) & (top > 0.0)
    s = np.full(tot.shape, QUIET)
    s[loud] = np.log10(top[loud] / tot[loud])
    return s, np.where(loud, ramp(s, s0, kappa), 0.0)


def update(r, eps_max, eps_prev, hold, cc4_base, scale, dtype=np.float64):
    """``(eps, cc4)``: the hold and the cell constant, formed in double and stored in ``dtype``; ``cc4_base`` where eps == 0."""
    eps = np.maximum(r * eps_max, hold * np.asarray(eps_prev, dtype=np.float64))
    base, sc = np.asarray(cc4_base, dtype=dtype), np.asarray(scale, dtype=dtype)
    cc4 = (base.astype(np.float64) - eps * sc.astype(np.float64)).astype(dtype)
    return eps, np.where(eps == 0.0, base, cc4)


def sensor(u, dofmap, P, floor, s0, kappa, eps_max, eps_prev=None, hold=0.0, dtype=np.float64):
    """One launch: ``dict(tot, top, btot, btop, s, r, eps)``."""
    tot, top, btot, btop = energies(table(P, dtype), u, dofmap, P, dtype)
    s, r = sense(tot, top, floor, s0, kappa)
    prev = np.zeros_like(tot) if eps_prev is None else eps_prev
    return dict(tot=tot, top=top, btot=btot, btop=btop, s=s, r=r, eps=np.maximum(r * eps_max, hold * prev))


def intervals(tot, top, btot, btop, floor, s0, kappa, eps_max, eps_prev, hold):
    """What the energy bounds allow the device: ``(s_lo, s_hi, eps_lo, eps_hi, decided)`` per cell.  ``s`` and ``r`` are monotone in
    ``top / tot``, so the ends of ``[top - b, top + b] / [tot + b, tot - b]`` bound them; a few ulps of double for the division, the
    logarithm and the sine are added, the ramp's largest slope pi / (4 kappa) carrying those of ``s`` into ``r``.  ``s_lo`` is -inf
    where ``top - b <= 0`` (the device may then hold the sentinel).  ``decided``: the quiet test ``tot <= 8 floor^2`` falls the same
    way at both ends of ``tot``'s interval."""
    f8 = 8.0 * floor * floor
    decided = (tot + btot <= f8) | (tot - btot > f8)
    quiet = tot <= f8
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(top - btop > 0.0, np.log10(np.maximum(top - btop, 1e-300) / (tot + btot)), -np.inf)
        hi = np.log10((top + btop) / np.maximum(tot - btot, 1e-300))
    ulps = 16 * U64
    lo, hi = lo - ulps * np.maximum(1.0, np.abs(lo)), hi + ulps * np.maximum(1.0, np.abs(hi))
    slack = ulps * (1.0 + np.pi / (4.0 * kappa) * np.maximum(1.0, np.abs(hi)))
    r_lo = np.where(quiet, 0.0, np.maximum(ramp(np.maximum(lo, -1e300), s0, kappa) - slack, 0.0))
    r_hi = np.where(quiet, 0.0, np.minimum(ramp(hi, s0, kappa) + slack, 1.0))
    prev = hold * np.asarray(eps_prev, dtype=np.float64)
    return lo, hi, np.maximum(r_lo * eps_max, prev), np.maximum(r_hi * eps_max, prev), decided


# ---- the run -------------------------------------------------------------------------------------------------------------------------
C0, RHO0, BETA, F0, ATT_DB = 1500.0, 1000.0, 3.5, 1.0e6, 0.2

# The two solver cases, chosen on this model.  P = 4, CFL 0.4 snapped to a whole number of steps per period.
# HIGH: 35 MPa at the source (the plane wave this source convention launches has amplitude 2 p0), h = lambda / 2, twelve periods.  The
# shock forms inside the box -- rho c^3 / (beta omega p0) = 4.4 mm of its 12 mm, 2.2 mm for the amplitude that travels -- at a
# resolution far too coarse for the physical delta.  ``overshoot_*``: max |u| / p0 - 1 over the steps of the plain run and of the run
# with the default attachment, from ``Run`` (tests/test_shock_capture.py recomputes both); a clean wave of this source reads 1.
# LOW: 10 kPa (shock distance 15 m), h = lambda / 3, six periods: every cell stays below the ramp or under the floor.
HIGH_DRIVE = dict(p0=35e6, ncells=16, length=0.012, dt=1.25e-8, steps=960, overshoot_plain=6.806710231837542,
                  overshoot_captured=2.820571814597209)
LOW_DRIVE = dict(p0=1e4, ncells=24, length=0.012, dt=1e-6 / 121, steps=726)


def shock_distance(p0, c=C0, rho=RHO0, beta=BETA, f0=F0):
    """rho c^3 / (beta omega p0): where a plane wave of amplitude p0 forms its shock."""
    return rho * c**3 / (beta * 2.0 * np.pi * f0 * p0)


def thin_box(ncells, length, P=4, grid=(1, 1, 1), rank=0, dtype=np.float64):
    """``ncells`` x 1 x 1 cubes of degree ``P`` along x: the rigid lateral walls keep a plane wave planar."""
    h = length / ncells
    return pkg("boxmesh").BoxMesh(P, (ncells, 1, 1), grid=grid, rank=rank, length=(length, h, h), dtype=dtype)


def cell_size(mesh):
    """The cube root of every cell's volume, from the oracle's detJ (it carries the quadrature weights)."""
    return np.cbrt(np.abs(rk4_oracle.host_detJ(mesh)).sum(axis=1))


class Run:
    """The CPU model of ``WesterveltSpectral3D(mesh, ..., shock_capture=ShockCapture(...)).rk4(0, ., dt, max_steps=nsteps)`` from rest.
    ``capture``: None (the plain run) or ``dict(eps_max=, s0=, kappa=, floor=, hold=, every=)``."""

    def __init__(self, mesh, p0, att_dB=0.2, capture=None, c0=C0, rho0=RHO0, beta=BETA, f0=F0):
        self.mesh, self.p0, self.att_dB, self.capture = mesh, float(p0), att_dB, capture
        self.c0, self.rho0, self.beta, self.f0 = c0, rho0, beta, f0
        self.geo = rk4_oracle.host_geometry(mesh)
        self.scale = np.full(mesh.ncells, 1.0 / (rho0 * c0 * c0))
        self.eps = np.zeros(mesh.ncells)
        self.sensor = np.full(mesh.ncells, QUIET)
        self.u, self.v, self.t, self.steps = np.zeros(mesh.ndofs), np.zeros(mesh.ndofs), 0.0, 0
        self.peak = 0.0  # max |u| over the steps so far
        self.max_eps = 0.0  # the largest eps any sensor evaluation has set so far

    def _source(self, t_off):
        """The model's uniform source at ``t_off + t`` (each ``solve_westervelt`` call counts its time from 0)."""
        f0, w0, p0, c0 = self.f0, 2 * np.pi * self.f0, self.p0, self.c0
        nd = self.mesh.ndofs

        def source_term(t, b, coefficients, detJ, dofmap):
            t = t_off + t
            T, alpha = 1 / f0, 4.0
            if t < T * alpha:
                window = 0.5 * (1 - np.cos(f0 * np.pi * t / alpha))
                dwindow = 0.5 * np.pi * f0 / alpha * np.sin(f0 * np.pi * t / alpha)
            else:
                window, dwindow = 1.0, 0.0
            a = 2 * p0 * w0 / c0
            oracle_np.mass_apply(np.full(nd, window * a * np.cos(w0 * t)), coefficients[0], b, detJ, dofmap)
            oracle_np.mass_apply(np.full(nd, dwindow * a * np.cos(w0 * t) - window * a * w0 * np.sin(w0 * t)), coefficients[1], b, detJ, dofmap)

        return source_term

    def _stage_term(self):
        if self.capture is None or not np.any(self.eps > 0.0):
            return None
        cc, Df, mesh, geo = -self.eps * self.scale, self.geo.D.flatten(), self.mesh, self.geo

        def bind(m0):
            def term(b, un, vn):  # K(cc4_base + d) = K(cc4_base) + K(d), exactly
                oracle_np.stiffness_apply(mesh.P, Df, np.ascontiguousarray(vn), cc, b, geo.G, mesh.dofmap)

            return term

        return bind

    def advance(self, nsteps, dt, observe=None):
        """``nsteps`` more steps of ``dt``, a segment of ``every`` steps between two sensor evaluations (the oracle's loop is called
        step by step, so that ``peak`` sees every step; the stage term of a segment is the same in each of its steps);
        ``observe(t, u)`` after each step if given.  Returns ``(u, v)``."""
        g = self.geo
        factors = (g.G, g.detJ, g.dF1, g.dF2)
        for _ in range(nsteps):
            self.u, self.v = rk4_oracle.solve_westervelt(
                self.mesh, 1, dt, c0=self.c0, rho0=self.rho0, f0=self.f0, p0=self.p0, beta=self.beta, att_dB=self.att_dB,
                geometry=factors, u=self.u, v=self.v, stage_term=self._stage_term(), source_term=self._source(self.t))
            self.steps, self.t = self.steps + 1, self.t + dt
            self.peak = max(self.peak, float(np.abs(self.u).max()))
            if observe is not None:
                observe(self.t, self.u)
            if self.capture is not None and self.steps % self.capture["every"] == 0:
                c = self.capture
                out = sensor(self.u, self.mesh.dofmap, self.mesh.P, c["floor"], c["s0"], c["kappa"], c["eps_max"], self.eps, c["hold"])
                self.eps, self.sensor = out["eps"], out["s"]
                self.max_eps = max(self.max_eps, float(self.eps.max()))
        return self.u, self.v


def default_capture(mesh, p0, strength=0.1, s0=None, kappa=0.5, floor=None, hold=0.0, every=1, c0=C0):
    """The attachment's defaults as the model's ``capture`` record."""
    P = mesh.P
    return dict(eps_max=strength * c0 * cell_size(mesh) / P**2, s0=-4.0 * np.log10(P) - 0.5 if s0 is None else s0, kappa=kappa,
                floor=0.03 * p0 if floor is None else floor, hold=hold, every=every)


@functools.lru_cache(maxsize=None)
def cached(fn, *args):
    """One evaluation of ``fn(*args)`` shared among the tests that need it."""
    return fn(*args)
