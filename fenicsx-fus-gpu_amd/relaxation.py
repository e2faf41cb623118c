"""
Power-law tissue absorption through relaxation mechanisms (memory variables) for both wave solvers (csrc/relaxation.hpp,
``fus_relax_stage_*``).

Soft tissue absorbs as ``alpha0 f^y`` with ``y`` between 1 and 1.5; the thermoviscous term of the Westervelt model gives ``f^2`` and
the linear model has no volume loss.  The time-domain remedy is a small set of relaxation mechanisms whose summed absorption fits
the power law over the band of interest: per owned dof and mechanism ``nu`` a memory variable

    xi_nu' = kappa_nu v - xi_nu / tau_nu                      (u' = v as before)

and every stiffness apply of a stage acts on ``ur = u_n + sum_nu xi_nu,n`` in the place of ``u_n``.  In the frequency domain the
stiffness sees ``u (1 + S(w))`` with ``S = sum_nu kappa_nu i w tau_nu / (1 + i w tau_nu)``; to first order in kappa

    alpha_r(w) = (w / 2c) sum_nu kappa_nu w tau_nu / (1 + w^2 tau_nu^2)                 [Np/m]
    c_ph(w)    = c (1 + 1/2 sum_nu kappa_nu w^2 tau_nu^2 / (1 + w^2 tau_nu^2))

so the solver's ``speed_of_sound`` is the EQUILIBRIUM (low-frequency) speed.  The thermoviscous ``delta`` of the Westervelt solver
stays as it is and adds its ``delta w^2 / (2 c^3)``.

    fit = fit_power_law(0.5, 1.1, 0.5e6, 5e6, n=2, speed_of_sound=1540.0)        # tau, kappa, delta, max_rel_error
    solver = LinearSpectral3D(mesh, ..., relaxation=RelaxationAbsorption(fit.tau, fit.kappa))

Per-tissue weights: call ``fit_power_law`` per tissue with the same ``tau`` and hand ``kappa`` over as ``[NR, ncells]``.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

MAX_MECHANISMS = 4  # csrc/relax_table.hpp: the mechanism count is a template parameter of the kernel
STABILITY_LIMIT = 2.785  # real-axis limit of the classical RK4: dt / min(tau) must stay below it
NP_PER_DB = np.log(10.0) / 20.0

PowerLawFit = namedtuple("PowerLawFit", "tau kappa delta max_rel_error")


class RelaxationAbsorption:
    """``NR`` relaxation mechanisms: times ``tau`` [NR] (global scalars, seconds) and weights ``kappa >= 0``, ``[NR]`` (a homogeneous
    medium: no per-dof vector is kept) or ``[NR, ncells]`` in the caller's cell order like the other material arrays (used per dof
    as the lumped average ``M(kappa_nu) 1 / M(1) 1``)."""

    def __init__(self, tau, kappa):
        self.tau = np.atleast_1d(np.asarray(tau, dtype=np.float64)).copy()
        self.kappa = np.asarray(kappa, dtype=np.float64).copy()
        nr = self.tau.size
        if self.tau.ndim != 1 or not 1 <= nr <= MAX_MECHANISMS:
            raise ValueError(f"tau: 1 to {MAX_MECHANISMS} relaxation times, got shape {self.tau.shape}")
        if not np.all(self.tau > 0.0) or not np.all(np.isfinite(self.tau)):
            raise ValueError("tau: every relaxation time must be positive")
        if self.kappa.ndim not in (1, 2) or self.kappa.shape[0] != nr:
            raise ValueError(f"kappa: shape [{nr}] or [{nr}, ncells], got {self.kappa.shape}")
        if not np.all(self.kappa >= 0.0):
            raise ValueError("kappa: the weights must be non-negative")
        self.nr = nr
        self.homogeneous = self.kappa.ndim == 1

    # -- the frequency-domain model ------------------------------------------------------------------------------------------
    def _wt(self, f):
        w = 2.0 * np.pi * np.asarray(f, dtype=np.float64)
        return w, w[..., None] * self.tau  # [..., NR]

    def _weights(self, kappa):
        return self.kappa if kappa is None else np.asarray(kappa, dtype=np.float64)

    def S(self, f, kappa=None):
        """``sum_nu kappa_nu i w tau_nu / (1 + i w tau_nu)`` (scalar weights: this object's, or ``kappa`` [NR])."""
        _, wt = self._wt(f)
        return np.sum(self._weights(kappa) * (1j * wt) / (1.0 + 1j * wt), axis=-1)

    def wavenumber(self, f, c, kappa=None):
        """The complex ``k(w) = (w / c) (1 + S)^(-1/2)`` of a plane wave ``e^{i (w t - k x)}``: ``alpha = -Im k``, ``c_ph = w / Re k``."""
        w, _ = self._wt(f)
        return w / c / np.sqrt(1.0 + self.S(f, kappa))

    def alpha(self, f, c, kappa=None):
        """``alpha_r`` in Np/m at frequency ``f`` (Hz) and equilibrium speed ``c``, to first order in kappa."""
        w, wt = self._wt(f)
        return w / (2.0 * c) * np.sum(self._weights(kappa) * wt / (1.0 + wt * wt), axis=-1)

    def phase_speed(self, f, c, kappa=None):
        """``c_ph`` at frequency ``f``, to first order in kappa; ``c`` is its low-frequency limit."""
        _, wt = self._wt(f)
        return c * (1.0 + 0.5 * np.sum(self._weights(kappa) * wt * wt / (1.0 + wt * wt), axis=-1))

    def check_time_step(self, dt):
        """``ValueError`` where the explicit RK4 cannot follow the fastest mechanism: ``dt / min(tau) >= 2.785``."""
        ratio = float(dt) / float(self.tau.min())
        if ratio >= STABILITY_LIMIT:
            raise ValueError(f"relaxation: dt / min(tau) = {ratio:.3f} >= {STABILITY_LIMIT} (the real-axis stability limit of RK4): "
                             "use a smaller time step or a larger relaxation time")

    # -- on the device ---------------------------------------------------------------------------------------------------------
    def cell_weights(self, mesh):
        """``[NR, ncells]`` in the MESH's cell order (per-cell weights only)."""
        from .solver_base import per_cell

        return np.stack([per_cell(self.kappa[nu], mesh, f"kappa[{nu}]") for nu in range(self.nr)])

    def bind_schedule(self, solver):
        """Generator: the state of one solver on its device -- ``xi0``, ``xin``, ``acc`` [NR, stride] (zero), ``ur`` and, for per-cell
        weights, the per-dof weights ``M(kappa_nu) 1 / M(1) 1`` (assembled with the solver's cell mass operator; a ``yield`` after
        posting each reverse exchange on a partitioned mesh).  Returns a ``BoundRelaxation``."""
        import torch

        from .field_monitor import dof_volumes_schedule, lumped_mass_schedule

        n, w = solver.nlocal, 16 // solver.tdt_np.itemsize
        stride = max(w, -(-n // w) * w)  # every row starts 16-byte aligned
        z = lambda: torch.zeros((self.nr, stride), dtype=solver.tdt, device=solver.dev)  # noqa: E731
        kappa_d, cells = None, None
        if not self.homogeneous:
            cells = self.cell_weights(solver.mesh)
            vol = yield from dof_volumes_schedule(solver)
            kappa_d = z()
            for nu in range(self.nr):
                mk = yield from lumped_mass_schedule(solver, cells[nu])
                kappa_d[nu, :n] = (mk / vol).to(solver.tdt)
        return BoundRelaxation(self, kappa_d, cells, z(), z(), z(), torch.zeros(solver.ndofs, dtype=solver.tdt, device=solver.dev), n)


class BoundRelaxation:
    """A ``RelaxationAbsorption`` on the device for one solver: what ``operators.relax_stage`` launches with."""

    def __init__(self, model, kappa_d, kappa_cells, xi0, xin, acc, ur, nlocal):
        self.model, self.tau, self.nr = model, model.tau, model.nr
        self.kappa = model.kappa if kappa_d is None else kappa_d  # host scalars [NR] or device [NR, stride]
        self.kappa_cells = kappa_cells  # [NR, ncells] in the mesh's cell order, or None
        self.xi0, self.xin, self.acc, self.ur, self.nlocal = xi0, xin, acc, ur, nlocal

    def state(self):
        return (self.ur, self.xi0, self.xin, self.acc)

    def zero(self):
        for t in self.state():
            t.zero_()

    def enter(self, u):
        """``ur = u + sum_nu xi0_nu`` over the owned dofs: before the first stage of a time loop."""
        n = self.nlocal
        self.ur[:n] = u[:n] + self.xi0[:, :n].sum(dim=0)

    def stage(self, kind, bw, aw, aw_u, u_base, vn):
        from . import operators as ops

        ops.relax_stage(bw, aw, aw_u, kind, self.tau, self.kappa, self.xi0, self.xin, self.acc, u_base, vn, self.ur, self.nlocal)


# -- the fit ---------------------------------------------------------------------------------------------------------------------
def fit_power_law(alpha0_dB_cm_MHzy, y, f_lo, f_hi, n=2, speed_of_sound=1540.0, with_thermoviscous=True, tau=None, samples=64):
    """Relaxation weights whose absorption fits ``alpha0 f^y`` (``alpha0`` in dB/cm/MHz^y) between ``f_lo`` and ``f_hi`` (Hz):
    ``n`` mechanisms with relaxation frequencies ``1 / (2 pi tau_nu)`` log-spaced from ``f_lo`` to ``f_hi`` (or the given ``tau``:
    per-tissue fits share one set of times), and a non-negative least-squares fit of the RELATIVE error at ``samples`` log-spaced
    frequencies; ``with_thermoviscous``: the diffusivity ``delta`` (its ``delta w^2 / (2 c^3)``) is among the unknowns.  Returns
    ``PowerLawFit(tau, kappa, delta, max_rel_error)``; ``delta`` is 0.0 without the thermoviscous term."""
    from scipy.optimize import nnls

    c = float(speed_of_sound)
    if not 0.0 < f_lo < f_hi:
        raise ValueError("fit_power_law: 0 < f_lo < f_hi")
    if tau is None:
        if not 1 <= n <= MAX_MECHANISMS:
            raise ValueError(f"fit_power_law: 1 to {MAX_MECHANISMS} mechanisms")
        fr = np.array([np.sqrt(f_lo * f_hi)]) if n == 1 else np.geomspace(f_lo, f_hi, n)
        tau = 1.0 / (2.0 * np.pi * fr)
    tau = np.atleast_1d(np.asarray(tau, dtype=np.float64))
    f = np.geomspace(f_lo, f_hi, samples)
    w = 2.0 * np.pi * f
    target = alpha0_dB_cm_MHzy * NP_PER_DB * 100.0 * (f / 1e6) ** y  # Np/m
    wt = w[:, None] * tau
    cols = [(w / (2.0 * c))[:, None] * wt / (1.0 + wt * wt)]
    if with_thermoviscous:
        cols.append((w * w / (2.0 * c**3))[:, None])
    A = np.hstack(cols)
    scale = A.max(axis=0)  # columns of very different size (kappa ~ 1e-3, delta ~ 1e-6): fit scaled unknowns
    x, _ = nnls(A / scale / target[:, None], np.ones(f.size))
    x = x / scale
    err = float(np.max(np.abs(A @ x / target - 1.0)))
    return PowerLawFit(tau, x[: tau.size].copy(), float(x[tau.size]) if with_thermoviscous else 0.0, err)


# -- absorbed power ---------------------------------------------------------------------------------------------------------------
def heat_deposition_schedule(monitor, solver):
    """Generator form of ``heat_deposition`` for a driver that advances several ranks from one process."""
    import torch

    from .field_monitor import dof_volumes_schedule, heat_deposition_schedule as thermoviscous, lumped_mass_schedule

    bound = getattr(solver, "_relax", None)
    if bound is None:
        raise ValueError("relaxation.heat_deposition: the solver has no relaxation= (field_monitor.heat_deposition is the thermoviscous part)")
    if not monitor.harmonics:
        raise ValueError("relaxation.heat_deposition: the monitor accumulates no harmonics (harmonics=(1, ...), frequency=f0)")
    q = torch.zeros(solver.nlocal, dtype=torch.float64, device=solver.dev)
    if hasattr(solver, "delta_cells"):
        q = q + (yield from thermoviscous(monitor, solver))
    vol = yield from dof_volumes_schedule(solver)
    model, nc = bound.model, solver.mesh.ncells
    kc = bound.kappa_cells if bound.kappa_cells is not None else np.repeat(model.kappa[:, None], nc, axis=1)
    for k in monitor.harmonics:
        wt = k * monitor.omega * model.tau
        alpha = k * monitor.omega / (2.0 * solver.c_cells) * ((wt / (1.0 + wt * wt)) @ kc)  # alpha_r(k w0) per cell, Np/m
        ma = yield from lumped_mass_schedule(solver, alpha / (solver.rho_cells * solver.c_cells))
        q = q + ma / vol * monitor.harmonic_amplitude(k) ** 2
    return q


def heat_deposition(monitor, solver):
    """The absorbed power density of a solver with ``relaxation=``: the thermoviscous ``field_monitor.heat_deposition`` where the
    solver has a ``delta``, plus, over the monitor's harmonics ``k``,

        sum_k (M(alpha_r(k w0) / (rho c)) 1 / M(1) 1) |P_k|^2

    This is the PLANE-WAVE form ``2 alpha I`` with ``I = |P|^2 / (2 rho c)`` per harmonic -- an approximation wherever the field is
    not a progressive plane wave (standing waves, the near field) -- with ``alpha_r`` the first-order absorption of the mechanisms
    per cell (of a solver with a nodal medium: from the per-cell means of its nodal rho and c, as its per-cell weights' lumped
    projection).  Torch math on the monitor's maps; device tensor [nlocal], fp64."""
    from .solver_base import run_schedule

    return run_schedule(heat_deposition_schedule(monitor, solver))
