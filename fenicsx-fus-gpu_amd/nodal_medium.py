"""
Nodal material fields: the medium given at the dofs instead of one value per cell.

A spectral element has material sample points at the resolution of its own dofs: the GLL quadrature is collocated, so a coefficient
at the dofs is a coefficient at the quadrature points -- n times finer per axis than the DG0 arrays of ``solver_base.per_cell`` on the
same mesh, with no remeshing and no smaller time step.  ``LinearSpectral3D(..., nodal_medium=NodalMedium(c, rho))`` takes one:

  stiffness     ``y += K(-1 * 1/rho) x`` with 1/rho inside the contraction (csrc/stiffness_geom_nodal.hpp,
                ``operators.stiffness_operator(..., geometry=..., nodal=1/rho)``), or, with ``in_kernel_geometry=False``, the general-G
                kernel on ``scale_G(G, 1/rho, dofmap)``
  lumped mass   ``(M(1) 1, reverse-scattered) * 1/(rho c^2)``: diagonal
  facet terms   one value per facet, the mean of the nodal coefficient over the facet's dofs

``WesterveltSpectral3D(..., nodal_medium=NodalMedium(c, rho, nonlinear_coefficient=beta, attenuation_coefficient_dB=alpha))`` takes the
four fields of the nonlinear solver (``evaluate_westervelt``): 1/rho and delta/(rho c^2) inside the two contractions of ONE cell pass
(csrc/westervelt_geom_nodal.hpp, ``operators.westervelt_cell_operator(..., geometry=, nodal=)``), three diagonals ``M(1) 1`` times a
nodal factor, one mean coefficient per facet.

``sample_volume`` turns a voxel map (a CT-derived c / rho volume) into such an array.  No reference counterpart: its drivers take
DG0 arrays only.
"""

from __future__ import annotations

import numpy as np
import torch


class NodalMedium:
    """``NodalMedium(speed_of_sound, density)``: each a scalar, an array with one value per LOCAL dof (owned and ghost dofs, in the
    mesh's numbering), or a callable ``f(xyz) -> [ndofs]`` evaluated on ``mesh.dof_coordinates()`` (``xyz`` is ``[ndofs, 3]``); a mesh
    without ``dof_coordinates`` accepts scalars and arrays only.

    On a partitioned mesh a ghost's value is computed by the rank that HOLDS it (from its own array or its own coordinates): nothing
    is exchanged, so the values a dof is given on different ranks must agree -- a callable of position, or arrays cut from one
    global field, do.  Non-finite and non-positive values raise.

    ``nonlinear_coefficient`` (beta) / ``attenuation_coefficient_dB`` (keywords, the Westervelt solver's fields; the linear solver
    ignores them): the same three forms, finite and >= 0 (water has beta > 0, a lossless region alpha = 0); ``None`` takes the
    solver's scalar (``evaluate_westervelt``)."""

    def __init__(self, speed_of_sound, density, *, nonlinear_coefficient=None, attenuation_coefficient_dB=None):
        self.speed_of_sound, self.density = speed_of_sound, density
        self.nonlinear_coefficient, self.attenuation_coefficient_dB = nonlinear_coefficient, attenuation_coefficient_dB

    @staticmethod
    def _field(value, mesh, name, xyz, positive=True):
        if callable(value):
            if xyz is None:
                raise ValueError(f"{name}: a callable needs mesh.dof_coordinates(), which {type(mesh).__name__} does not have: "
                                 "pass one value per local dof")
            a = np.asarray(value(xyz), dtype=np.float64)
            if a.shape != (mesh.ndofs,):
                raise ValueError(f"{name}: the callable must return one value per local dof ({mesh.ndofs}), got shape {a.shape}")
        else:
            a = np.asarray(value, dtype=np.float64)
            if a.ndim == 0:
                a = np.full(mesh.ndofs, float(a))
            elif a.shape != (mesh.ndofs,):
                raise ValueError(f"{name}: a scalar, a callable of xyz or one value per local dof, owned and ghost ({mesh.ndofs}), "
                                 f"got shape {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{name}: non-finite nodal values")
        if positive and not np.all(a > 0.0):
            raise ValueError(f"{name}: nodal values must be positive (min {a.min()})")
        if not positive and not np.all(a >= 0.0):
            raise ValueError(f"{name}: nodal values must not be negative (min {a.min()})")
        return np.ascontiguousarray(a)

    def evaluate(self, mesh):
        """``(c, rho)``: float64 arrays ``[mesh.ndofs]`` in the mesh's dof numbering."""
        need_xyz = callable(self.speed_of_sound) or callable(self.density)
        xyz = mesh.dof_coordinates() if need_xyz and hasattr(mesh, "dof_coordinates") else None
        return (self._field(self.speed_of_sound, mesh, "speed_of_sound", xyz), self._field(self.density, mesh, "density", xyz))

    def evaluate_westervelt(self, mesh, nonlinear_coefficient=None, attenuation_coefficient_dB=None):
        """``(c, rho, beta, att_dB)``: float64 arrays ``[mesh.ndofs]`` in the mesh's dof numbering.  The two arguments are the
        scalars a field left ``None`` takes (the solver passes its own); a field that is ``None`` in both places raises."""
        fields = []
        for name, own, default in (("nonlinear_coefficient", self.nonlinear_coefficient, nonlinear_coefficient),
                                   ("attenuation_coefficient_dB", self.attenuation_coefficient_dB, attenuation_coefficient_dB)):
            if own is None:
                if default is None or np.ndim(default) != 0:
                    raise ValueError(f"{name}: the medium leaves it None, so a scalar must be given")
                own = default
            xyz = mesh.dof_coordinates() if callable(own) and hasattr(mesh, "dof_coordinates") else None
            fields.append(self._field(own, mesh, name, xyz, positive=False))
        return self.evaluate(mesh) + tuple(fields)


def cell_means(nodal, dofmap):
    """Per-cell mean of a nodal array over the dofs of each cell (what ``rho_cells`` / ``c_cells`` of a solver with a nodal medium hold)."""
    return np.asarray(nodal, dtype=np.float64)[np.asarray(dofmap)].mean(axis=1)


def facet_means(nodal, facet_dofmap):
    """The facet rule: one coefficient per facet, the mean of the nodal coefficient over that facet's dofs (exact where the medium
    is constant on the facet)."""
    fd = np.asarray(facet_dofmap)
    if fd.shape[0] == 0:
        return np.zeros(0)
    return np.asarray(nodal, dtype=np.float64)[fd].mean(axis=1)


def scale_G(G, kappa, dofmap):
    """The pre-scaled geometric factor ``G'[c, q, :] = kappa[dofmap[c, q]] G[c, q, :]`` for the general-G kernels, formed where G lives
    (the device, for the solvers' G; set-up, once):
    ``stiffness_operator(P, dphi, ft)(x, cc, y, G', dofmap)`` is then ``y += K(cc * kappa) x``, the operator of the nodal kernel (which
    reads no G array: this one is 6 n^3 values per cell).  ``G``: device tensor ``[ncell, n^3, 6]``; ``kappa``: one value per dof (host
    array or device tensor); ``dofmap``: ``[ncell, n^3]``.  Returns a new tensor of G's type."""
    if not isinstance(G, torch.Tensor):
        raise TypeError(f"scale_G: G must be a torch.Tensor (the solvers' device array), got {type(G).__name__}")
    dm = dofmap if isinstance(dofmap, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dofmap))
    dm = dm.to(G.device).long()
    k = kappa if isinstance(kappa, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(kappa))
    k = k.to(device=G.device, dtype=G.dtype).reshape(-1)
    if G.dim() != 3 or G.shape[2] != 6 or tuple(dm.shape) != tuple(G.shape[:2]):
        raise ValueError("scale_G: G must be [ncell, n^3, 6] and dofmap [ncell, n^3]")
    if dm.numel() and not 0 <= int(dm.min()) <= int(dm.max()) < k.numel():
        raise ValueError(f"scale_G: kappa has {k.numel()} entries, the dofmap refers to dofs up to {int(dm.max())}")
    return (G * k[dm].unsqueeze(-1)).contiguous()


def sample_volume(volume, origin, spacing, xyz):
    """Trilinear samples of a voxel map at points (numpy, set-up time): ``volume[i, j, k]`` is the value AT
    ``origin + (i, j, k) * spacing``; a point outside the volume takes the value at the nearest point of its faces (coordinates are
    clamped).  ``xyz``: ``[npts, 3]`` (``mesh.dof_coordinates()``); returns ``[npts]`` float64.  This is how a CT-derived c / rho map
    becomes the nodal array of ``NodalMedium``."""
    vol = np.asarray(volume, dtype=np.float64)
    if vol.ndim != 3 or min(vol.shape) < 1:
        raise ValueError("sample_volume: volume must be a non-empty 3-D array")
    pts = np.asarray(xyz, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("sample_volume: xyz must be [npts, 3]")
    sp = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
    if not np.all(sp > 0.0):
        raise ValueError("sample_volume: spacing must be positive")
    og = np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,))
    idx, frac = [], []
    for a in range(3):
        g = np.clip((pts[:, a] - og[a]) / sp[a], 0.0, vol.shape[a] - 1.0)
        i0 = np.minimum(np.floor(g).astype(np.int64), max(vol.shape[a] - 2, 0))
        idx.append((i0, np.minimum(i0 + 1, vol.shape[a] - 1)))
        frac.append(g - i0)
    out = np.zeros(pts.shape[0])
    for bx in (0, 1):
        wx = frac[0] if bx else 1.0 - frac[0]
        for by in (0, 1):
            wy = frac[1] if by else 1.0 - frac[1]
            for bz in (0, 1):
                wz = frac[2] if bz else 1.0 - frac[2]
                out += wx * wy * wz * vol[idx[0][bx], idx[1][by], idx[2][bz]]
    return out
