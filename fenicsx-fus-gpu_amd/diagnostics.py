"""
Run diagnostics of the two wave solvers on the device, built on the reduction kernel (reductions.py, csrc/reduce.hpp):

``EnergyRecorder``   the quadratic form the semi-discrete system ``M v' = -K u - C v + s`` conserves, ``E = 1/2 v^T M v + 1/2 u^T K u``,
                     after recorded steps -- ``M`` the lumped mass the stage kernel divides by (``m`` of the linear solver, ``m0`` of
                     Westervelt), ``K`` the stiffness with ``1/rho``.  One stiffness apply into a scratch vector of the recorder's
                     and one reduction launch pair per record, written straight into a device series: no host sync, no copy of a field.
``FieldGuard``       ``max |u|`` and the number of non-finite values every few steps, read back (the one sync), with an error that
                     names the step instead of NaNs coming back from ``u_sol()`` at the end.

Both are handed to ``rk4`` / ``rk4_schedule`` / ``rk4_graph`` (``energy=``, ``guard=``); absent, every launch stays as it is.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import operators as ops
from .reductions import Reducer


class EnergyRecorder:
    """``EnergyRecorder(solver, every=1, capacity=4096)``: records after every ``every``-th step that ends after ``record_from``
    (counted over the recorder's life, so that a run cut into several ``rk4`` calls keeps its cadence; ``reset`` restarts it) while
    the series has room; a full series stops recording and the run goes on.

    A record is one stiffness apply of ``u`` -- the solver's own operator, whichever form it holds (per-cell, geometry formed in the
    kernel, affine, nodal), into a scratch vector this recorder owns, zeroed first, never the solver's ``b`` -- and one
    ``Reducer.terms`` launch pair with ``sum0 = (v, v, M)``, ``sum1 = (u, y, None)``, ``x = u`` into row ``k`` of the device series
    ``[capacity, 4]``: ``v^T M v``, ``u . y``, ``max |u|``, the number of non-finite values.  With the solvers' sign convention the cell
    constants are ``-1/rho``, the apply yields ``y = -K u`` and the potential part is ``-1/2 u . y``.  The times are kept on the host.

    For ``WesterveltSpectral3D`` this is the energy of the LINEAR part: it decays with the diffusivity and is exchanged by the
    nonlinear term -- a diagnostic there, not an invariant.  With relaxation mechanisms the stiffness acts on ``u`` alone here.

    On a partitioned mesh the apply goes through the halo schedule (a forward exchange of ``u``, a reverse exchange of ``y``; it yields
    where ``HaloApply`` yields) and each rank records the sums over its owned dofs; ``energies`` adds the ranks' rows."""

    def __init__(self, solver, every=1, capacity=4096):
        self.every, self.capacity = int(every), int(capacity)
        if self.every < 1 or self.capacity < 1:
            raise ValueError(f"EnergyRecorder: every = {every}, capacity = {capacity}: both >= 1")
        self.solver = solver
        self._red = Reducer(solver.dev)
        self._y = torch.zeros(solver.ndofs, dtype=solver.tdt, device=solver.dev)
        self._rows = torch.zeros((self.capacity, 4), dtype=torch.float64, device=solver.dev)
        self.reset()

    def reset(self):
        """Forget the series and restart the cadence."""
        self.nrec, self._seen, self._times = 0, 0, []

    @property
    def full(self):
        return self.nrec >= self.capacity

    def expect_steps(self, start_time, final_time, dt, max_steps=None, record_from=None):
        """Nothing to upload: a record reads no per-step factors (the time loops announce their steps to every recorder)."""

    def record_schedule(self, u, v, t):
        """Generator: a step ending at ``t`` has left ``(u, v)``; record it if it is this recorder's turn."""
        self._seen += 1
        if self._seen % self.every or self.full:
            return
        s = self.solver
        ops.fill(0.0, self._y)
        yield from s._stiffness_of(u, self._y)
        self._red.terms(sum0=(v, v, s._energy_mass()), sum1=(u, self._y, None), x=u, n=s.nlocal, out=self._rows[self.nrec])
        self._times.append(float(t))
        self.nrec += 1

    def record(self, u, v, t):
        for _ in self.record_schedule(u, v, t):
            pass

    def rows(self):
        """This rank's series on the host, ``[nrec, 4]``: ``v^T M v``, ``u . y`` (``= -u^T K u``), ``max |u|``, non-finite count."""
        return self._rows[: self.nrec].cpu().numpy()

    def energies_schedule(self, reduce=None):
        """Generator form of ``energies`` (it yields after depositing this rank's rows in ``reduce``)."""
        rows = self.rows()
        every = yield from self.solver._gather(rows.reshape(-1), reduce, 0)
        every = np.asarray(every).reshape(len(every), -1, 4)
        total = every.sum(axis=0)
        kinetic, potential = 0.5 * total[:, 0], -0.5 * total[:, 1]
        return np.asarray(self._times), kinetic, potential, kinetic + potential, every[:, :, 2].max(axis=0), total[:, 3]

    def energies(self, reduce=None):
        """``(t, kinetic, potential, total, absmax, nonfinite)`` as host arrays, one entry per record.  On a partitioned mesh the
        ranks' rows are added (``absmax``: their maximum) through ``scatterer.gather_floats``, or through an ``InProcessGather`` passed
        as ``reduce=`` for ranks driven from one process (drive their ``energies_schedule`` in lock step)."""
        from .solver_base import run_schedule

        return run_schedule(self.energies_schedule(reduce))


class FieldGuard:
    """``FieldGuard(every=64, limit=inf)``: every ``every`` steps (counted over the guard's life; ``reset`` restarts the count) one
    ``Reducer.terms`` launch pair with ``x = u`` over the owned dofs, read back -- the one host sync -- and a ``FusGpuError`` if any
    value is not finite or ``max |u| > limit``.  The error names the step, the time and the value and, where an earlier
    ``stable_time_step`` call has made the limit known, ``dt`` against that limit.

    Ranks do not vote: a rank whose own dofs trip raises, and the others learn of it through the halo health check (their waits for
    the rank that left are bounded, and ``rk4`` raises on a failed exchange)."""

    def __init__(self, every=64, limit=np.inf):
        self.every, self.limit = int(every), float(limit)
        if self.every < 1 or not self.limit > 0.0:
            raise ValueError(f"FieldGuard: every = {every}, limit = {limit}: every >= 1 and limit > 0")
        self._red, self._dt = None, None
        self.reset()

    def reset(self):
        self.steps, self.last = 0, None  # steps seen; (absmax, nonfinite) of the last check

    def expect_steps(self, start_time, final_time, dt, max_steps=None, record_from=None):
        self._dt = float(dt)

    def check(self, solver, u, t):
        """A step ending at ``t`` has left ``u``."""
        self.steps += 1
        if self.steps % self.every:
            return
        if self._red is None or self._red.dev != u.device:
            self._red = Reducer(u.device)
        self.last = amax, bad = self._red.absmax(u, n=solver.nlocal)
        if bad or amax > self.limit:
            what = f"{bad} value(s) of u are not finite" if bad else f"max |u| = {amax:g} exceeds the limit {self.limit:g}"
            if bad:
                what += f" (largest finite |u| = {amax:g})"
            dt, limit = self._dt, solver.stable_limit
            if dt is not None and limit is not None:
                what += f"; dt = {dt:g} s against the RK4 stability limit {limit:g} s of stable_time_step(1)" + (
                    ": the step is too long" if dt > limit else "")
            rank = f" on rank {solver.comm.rank}" if solver.halo is not None else ""
            raise _lib.FusGpuError(f"FieldGuard: step {self.steps}, t = {t:g} s{rank}: {what}")
