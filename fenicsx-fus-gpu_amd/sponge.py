"""
Absorbing sponge layers for the two wave solvers (``LinearSpectral3D`` / ``WesterveltSpectral3D``, ``sponge=``).

The reference ends its domain with a first-order absorbing condition on ONE tagged face and rigid walls everywhere else; a
focused field leaves through the lateral faces too, at oblique incidence, and comes back from there.  The layer is the damped
wave equation

    u'' + 2 sigma u' + sigma^2 u = (undamped right-hand side),        sigma(x) >= 0, zero outside the layer

-- substituting ``u = exp(-sigma t) w`` shows that a constant sigma damps without changing the wave speed, so the layer's inner
edge does not reflect.  With GLL collocation the mass is diagonal, so per owned dof ``j`` of the layer a stage's right-hand side gets

    b[j] -= cv[j] v_n[j] + cu[j] u_n[j]          cv = 2 sigma_j m_j,   cu = sigma_j^2 m_j

with ``(u_n, v_n)`` the stage's inputs and ``m`` the solver's assembled lumped mass (the linear solver's ``m``; the Westervelt
solver's steady part ``m0``, which DEFINES its effective damping as ``2 sigma m0 / (m0 + w2 u_n)``).  One sparse launch per stage
over the layer's dofs (csrc/sponge.hpp, ``operators.sponge_terms``), placed with the facet terms; the vector pass that follows
divides by the mass exactly as it does without a layer.

Nothing enforces a time-step bound: the eigenvalues move from ``+- i omega`` to ``-sigma +- i omega``, and ``sigma_max dt`` must
stay well inside RK4's real-axis limit of 2.785 (``SpongeLayer.sigma_max`` is there to check).

``build`` is host numpy and needs no GPU.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import operators as ops

# faces of the box by name -> (axis, side); LATERAL: the four faces the reference leaves rigid around its x-directed beam
FACES = {"-x": (0, 0), "+x": (0, 1), "-y": (1, 0), "+y": (1, 1), "-z": (2, 0), "+z": (2, 1)}
LATERAL = ("-y", "+y", "-z", "+z")


def sigma_max_of(thickness, speed_of_sound, order=2, reflection=1e-4):
    """``-(order + 1) c ln(reflection) / (2 L)``: the usual estimate -- normal incidence, a round trip through a layer of width
    ``L`` with the profile ``sigma_max (d / L)^order`` attenuates by ``reflection``."""
    return -(order + 1) * float(speed_of_sound) * np.log(float(reflection)) / (2.0 * float(thickness))


def box_profile(lower, upper, thickness, faces, speed_of_sound, order=2, reflection=1e-4):
    """The callable ``sigma(xyz)`` (``xyz``: [npoints, 3]) of a layer of width ``thickness`` (a scalar, or one per axis) inside the
    chosen ``faces`` (names of ``FACES``) of the box ``[lower, upper]``: per face, with ``d`` the depth into the layer of width ``L``,
    ``sigma = sigma_max (d / L)^order`` and ``sigma_max = sigma_max_of(L, ...)``; where layers overlap, the maximum.  ``lower`` /
    ``upper`` are the GLOBAL box corners, so every rank of a partitioned mesh computes the same function."""
    lo, hi = (np.broadcast_to(np.asarray(a, dtype=np.float64), (3,)).copy() for a in (lower, upper))
    width = np.broadcast_to(np.asarray(thickness, dtype=np.float64), (3,)).copy()
    faces = tuple(faces)
    for f in faces:
        if f not in FACES:
            raise ValueError(f"box_profile: unknown face {f!r} (one of {sorted(FACES)})")
    axes = {FACES[f][0] for f in faces}
    if not np.all(hi > lo) or any(not (0.0 < width[a] <= hi[a] - lo[a]) for a in axes):
        raise ValueError("box_profile: needs lower < upper and 0 < thickness <= the box's extent")
    if order < 0 or not (0.0 < reflection < 1.0) or not speed_of_sound > 0:
        raise ValueError("box_profile: needs order >= 0, 0 < reflection < 1, speed_of_sound > 0")

    def sigma(xyz):
        xyz = np.asarray(xyz, dtype=np.float64)
        out = np.zeros(xyz.shape[0])
        for f in faces:
            a, side = FACES[f]
            L = width[a]
            depth = ((lo[a] + L) - xyz[:, a] if side == 0 else xyz[:, a] - (hi[a] - L)) / L
            # the layer's edge is a cell boundary in every use here: a depth of a few ulp there is the edge itself, not the layer
            depth = np.where(depth < 1e-12, 0.0, np.minimum(depth, 1.0))
            np.maximum(out, sigma_max_of(L, speed_of_sound, order, reflection) * depth**order * (depth > 0), out=out)
        return out

    return sigma


class SpongeLayer:
    """``sigma``: a callable ``sigma(xyz)`` (``box_profile``), evaluated on ``mesh.dof_coordinates()[:nlocal]``, or an array with one
    value per owned dof (a mesh handed over as arrays -- ``dolfinx_adaptor.ArrayMesh`` -- has no ``dof_coordinates()``).  Negative
    or non-finite values raise."""

    def __init__(self, sigma):
        if not callable(sigma):
            sigma = np.array(sigma, dtype=np.float64)
            if sigma.ndim != 1:
                raise ValueError(f"SpongeLayer: sigma must be a callable or a 1-D array (one value per owned dof), got shape {sigma.shape}")
            self._check(sigma)
        self.sigma = sigma
        self.sigma_max = None

    @staticmethod
    def _check(values):
        if not np.all(np.isfinite(values)) or np.any(values < 0):
            raise ValueError("SpongeLayer: sigma must be finite and >= 0 everywhere")

    def build(self, mesh):
        """Host: ``(idx, sigma)`` -- the ascending local indices (int32) of this rank's OWNED dofs with sigma > 0 and their sigma
        (float64); sets ``sigma_max`` (of this rank's list; 0 for an empty one).  Owned dofs only: each dof of a partitioned mesh is
        in exactly one rank's list, and the term needs no exchange."""
        nlocal = int(mesh.nlocal)
        if callable(self.sigma):
            values = np.asarray(self.sigma(np.asarray(mesh.dof_coordinates())[:nlocal]), dtype=np.float64).reshape(-1)
        else:
            values = self.sigma
        if values.shape != (nlocal,):
            raise ValueError(f"SpongeLayer: sigma has {values.size} values, the mesh owns {nlocal} dofs")
        self._check(values)
        idx = np.nonzero(values > 0)[0].astype(np.int32)  # np.nonzero ascends
        sig = np.ascontiguousarray(values[idx])
        self.sigma_max = float(sig.max()) if sig.size else 0.0
        self.built = (idx, sig)
        return self.built

    def bind(self, solver_mass, dtype, device, built=None):
        """The device triple ``(idx, cu, cv)`` of ``operators.sponge_terms``: ``cv = 2 sigma m``, ``cu = sigma^2 m`` with ``m =
        solver_mass[idx]`` -- the solver's assembled lumped mass, COMPLETE (after its reverse exchange) -- formed in fp64 and rounded
        to ``dtype`` once.  ``built``: the ``(idx, sigma)`` of ``build`` (default: the last one built)."""
        idx, sig = self.built if built is None else built
        _lib.require_device_tensor(solver_mass, solver_mass.dtype, "solver_mass")
        idx_d = torch.from_numpy(idx).to(device)
        sig_d = torch.from_numpy(sig).to(device)
        m = solver_mass.index_select(0, idx_d.long()).to(torch.float64)
        cv = ((2.0 * sig_d) * m).to(dtype).contiguous()
        cu = ((sig_d * sig_d) * m).to(dtype).contiguous()
        return idx_d, cu, cv


class SpongeTerm:
    """A ``SpongeLayer`` as a stage term of one solver (solver_base): its list of the rank's owned layer dofs is built at construction
    (host); its coefficients need the COMPLETE lumped mass, so ``bound`` -- ``(idx, cu, cv)`` -- stays None until the solver's set-up
    exchange has run.  Every argument of the launch is a fixed pointer: a captured step replays it."""

    capturable = True

    def __init__(self, layer, mesh):
        self.layer, self.built, self.bound = layer, layer.build(mesh), None

    def bind(self, solver, mass):
        self.bound = self.layer.bind(mass, solver.tdt, solver.dev, built=self.built)

    def launch(self, b, u_n, v_n, t):
        """b[j] -= cv[j] v_n[j] + cu[j] u_n[j] over the layer's owned dofs."""
        if self.bound is None:
            raise _lib.FusGpuError("sponge layer: the set-up exchange (setup_schedule) has not run, the layer is not bound yet")
        ops.sponge_terms(b, u_n, v_n, self.bound)
