"""
Shock capturing for ``WesterveltSpectral3D``: a per-cell smoothness sensor adds artificial diffusivity where the wave steepens
(``fus_modal_sensor_*``, csrc/modal_sensor.hpp, include/fus_gpu_sensor.h).

    cap = ShockCapture(strength=0.1)
    solver = WesterveltSpectral3D(mesh, ..., fused=True, shock_capture=cap)
    solver.rk4(...)                    # also rk4_graph(...)
    cap.artificial_diffusivity()       # [ncells], m^2/s, caller's cell order
    cap.sensor()                       # [ncells], log10 of the top modes' share of the cell's energy
    cap.active_cells()                 # how many cells carry eps > 0 (one sync)

At high drive the physical shock is far thinner than a cell and the spectral element rings.  The sensor (Persson-Peraire) is the
share of the cell's energy in its highest Legendre modes: it falls like P^-4 for a resolved field and stays O(1) at a front.  Above
the ramp around ``s0`` the cell gets ``eps_max = strength c h / P^2`` of diffusivity on top of its physical ``delta``, through the
cell constant the Westervelt cell pass already reads for ``K(delta / (rho c^2)) v``: one number per cell, written in place into
``solver.cc4`` after a step, so no kernel, stage kind or exchange of the solver changes and the pointers a captured graph holds stay.
A smooth cell keeps its constant bit for bit.  The field is never written.  There is no CPU fallback.
"""

from __future__ import annotations

import numpy as np
import torch
from numpy.polynomial import legendre as _leg

from . import _lib
from .gll import tabulate_1d

# what ``sensor()`` holds for a quiet cell: the header's sentinel (an infinity is never written)
QUIET = float(_lib._read_header([p for p in _lib.LATER_HEADER_PATHS if p.endswith("fus_gpu_sensor.h")][0])[1]["FUS_SENSOR_QUIET"])


def vandermonde(P):
    """``V[j][k] = sqrt((2k + 1) / 2) P_k(xi_j)``, fp64: the orthonormal Legendre basis on [-1, 1] at the degree-``P`` nodes in the
    order ``gll.tabulate_1d(P)`` returns them (whatever that order is)."""
    xi = 2.0 * np.asarray(tabulate_1d(P)[0], dtype=np.float64) - 1.0
    return np.stack([np.sqrt((2 * k + 1) / 2.0) * _leg.Legendre.basis(k)(xi) for k in range(P + 1)], axis=1)


def modal_table(P):
    """``Vinv`` [mode, node], fp64: the inverse of ``vandermonde(P)`` -- the true inverse, not ``V^T W`` (the GLL rule does not
    integrate ``P_P^2`` exactly)."""
    return np.ascontiguousarray(np.linalg.inv(vandermonde(P)))


# the default ``floor`` as a fraction of the source amplitude (calibrated on the CPU model: DESIGN 3.18)
DEFAULT_FLOOR = 0.03


def default_s0(P):
    """The centre of the default ramp.  A resolved field's top share falls like P^-4; with the default half-width 1/2 the ramp runs
    from ``-4 log10 P - 1`` (below it a cell gets exactly nothing) to ``-4 log10 P``, which a step anywhere inside a cell exceeds at
    every degree (DESIGN 3.18 has the table)."""
    return -4.0 * np.log10(P) - 0.5


class ShockCapture:
    """``ShockCapture(strength=0.1, s0=None, kappa=0.5, floor=None, hold=0.0, every=1, max_diffusivity=None)``.

    ``strength``          ``eps_max = strength c h / P^2`` per cell, ``h`` the cube root of the cell's volume, ``c`` its speed of sound
    ``max_diffusivity``   a scalar or one value per cell (caller's cell order) in m^2/s, in place of that
    ``s0``, ``kappa``     centre (default ``-4 log10 P - 1/2``) and half-width of the sine ramp in ``s = log10(top / tot)``
    ``floor``             a cell whose rms is at most this (Pa; default 0.03 of the source amplitude) is quiet: no diffusivity.  The
                          foot of a wave front entering a cell reads s = -1 .. -3 at any amplitude and on any mesh
    ``hold``              in [0, 1]: ``eps`` decays by this factor per sensor launch instead of dropping at once
    ``every``             a sensor launch after every ``every``-th step, counted over the attachment's life (``reset`` restarts it)

    Handed to ``WesterveltSpectral3D(shock_capture=)``, which binds it; one attachment serves one solver."""

    def __init__(self, strength=0.1, s0=None, kappa=0.5, floor=None, hold=0.0, every=1, max_diffusivity=None):
        self.strength, self.kappa, self.hold, self.every = float(strength), float(kappa), float(hold), int(every)
        self.s0 = None if s0 is None else float(s0)
        self.floor = None if floor is None else float(floor)
        self.max_diffusivity = max_diffusivity
        if not self.strength >= 0.0 or not self.kappa > 0.0 or not 0.0 <= self.hold <= 1.0 or self.every < 1:
            raise ValueError(f"ShockCapture: strength = {strength} (>= 0), kappa = {kappa} (> 0), hold = {hold} (0 .. 1), every = {every} (>= 1)")
        if self.floor is not None and not self.floor >= 0.0:
            raise ValueError(f"ShockCapture: floor = {floor}: >= 0")
        self.solver, self.steps, self.launches = None, 0, 0

    # -- binding ---------------------------------------------------------------------------------------------------------------------
    def bind(self, solver):
        """Called by the solver's constructor once ``cc1`` (``1 / (rho c^2)``), ``cc4``, ``detJ`` and ``dofmap`` are on the device."""
        from .solver_base import per_cell

        if self.solver is not None:
            raise ValueError("ShockCapture: already bound to a solver; one attachment serves one solver")
        self.solver = solver
        P, mesh, dev, tdt = solver.P, solver.mesh, solver.dev, solver.tdt
        self._fn = getattr(_lib.load(), f"fus_modal_sensor_{_lib.suffix(tdt)}")
        if self.s0 is None:
            self.s0 = float(default_s0(P))
        if self.floor is None:
            self.floor = DEFAULT_FLOOR * abs(float(solver.p0))
        if self.max_diffusivity is None:
            volume = solver.detJ.to(torch.float64).abs().sum(dim=1).cpu().numpy()  # detJ carries the quadrature weights
            eps_max = self.strength * np.asarray(solver.c_cells, dtype=np.float64) * np.cbrt(volume) / P**2
        else:
            eps_max = per_cell(self.max_diffusivity, mesh, "max_diffusivity")
        if eps_max.shape != (mesh.ncells,) or not np.all(np.isfinite(eps_max)) or np.any(eps_max < 0.0):
            raise ValueError("ShockCapture: the largest diffusivity of every cell must be finite and >= 0")
        self.eps_max = np.ascontiguousarray(eps_max, dtype=np.float64)  # the mesh's cell order
        self._eps_max = torch.from_numpy(self.eps_max).to(dev)
        self._Vinv = torch.from_numpy(modal_table(P).astype(solver.tdt_np)).to(dev)
        self._base, self._scale, self._cc4 = solver.cc4.clone(), solver.cc1, solver.cc4
        self._eps = torch.zeros(mesh.ncells, dtype=torch.float64, device=dev)
        self._sensor = torch.full((mesh.ncells,), QUIET, dtype=torch.float64, device=dev)
        return self

    def reset(self):
        """Forget the diffusivity (``cc4`` is the physical constant again) and restart the cadence; ``solver.init()`` calls this."""
        self.steps = self.launches = 0
        if self.solver is not None:
            self._eps.zero_()
            self._sensor.fill_(QUIET)
            self._cc4.copy_(self._base)

    # -- the time loop ---------------------------------------------------------------------------------------------------------------
    def due(self):
        """A step has ended: is a sensor launch due after it?"""
        self.steps += 1
        return self.steps % self.every == 0

    def launch(self, u):
        """One sensor launch on ``u`` (whose ghost entries must be current) on the current stream: ``eps``, ``sensor`` and the
        solver's ``cc4`` for the following steps.  No host sync."""
        s = self.solver
        _lib.require_device_tensor(u, s.tdt, "u")
        _lib.check(self._fn(u.data_ptr(), s.dofmap.data_ptr(), self._Vinv.data_ptr(), self._base.data_ptr(), self._scale.data_ptr(),
                            self._eps_max.data_ptr(), self._eps.data_ptr(), self._sensor.data_ptr(), self._cc4.data_ptr(), s.P,
                            s.mesh.ncells, self.s0, self.kappa, self.floor, self.hold, _lib.stream_ptr()), "fus_modal_sensor")
        self.launches += 1

    # -- what it found ---------------------------------------------------------------------------------------------------------------
    def _bound(self):
        if self.solver is None:
            raise _lib.FusGpuError("ShockCapture: not bound to a solver yet (WesterveltSpectral3D(shock_capture=...))")
        return self.solver

    def _caller_order(self, a):
        perm = getattr(self._bound().mesh, "cell_permutation", None)
        if perm is None:
            return a
        out = np.empty_like(a)
        out[np.asarray(perm)] = a  # the mesh's cell c is the caller's cell perm[c]
        return out

    def artificial_diffusivity(self):
        """``eps`` per cell in m^2/s after the last launch, on the host, caller's cell order."""
        self._bound()
        return self._caller_order(self._eps.cpu().numpy())

    def largest_diffusivity(self):
        """``eps_max`` per cell in m^2/s, on the host, caller's cell order."""
        self._bound()
        return self._caller_order(self.eps_max.copy())

    def sensor(self):
        """``log10(top / tot)`` per cell after the last launch (``QUIET`` = FUS_SENSOR_QUIET where the cell was quiet), on the
        host, caller's cell order."""
        self._bound()
        return self._caller_order(self._sensor.cpu().numpy())

    def active_cells(self):
        """How many of this rank's cells carry ``eps > 0`` (one sync)."""
        self._bound()
        return int((self._eps > 0.0).sum().item())

