"""numpy restatement of the weak gradient operator (csrc/gradient_geom.hpp) and of the maps of intensity.py: the per-point
quantities from ``(x_dofs, x_g, pts, wts, dphi)``, the scatter-add to three vectors, and ``recovered_gradient``, ``intensity_of``,
``radiation_force``.  The conventions are those of the reference's ``compute_scaled_geometrical_factor``: trilinear cells with vertex
``v = vx + 2 vy + 4 vz``, ``J_[a][d] = d x_d / d xi_a``, the tensor GLL rule ``q = qx n^2 + qy n + qz`` (= the local dof order);
tests/test_gradient.py anchors them to the reference's own ``detJ``, ``G`` and stiffness result.  Every array is computed in
``dtype`` (fp64 by default; fp32 to measure what the number format alone costs)."""

import numpy as np


def p1_gradients(pts, dtype=np.float64):
    """``[3, nq, 8]``: d N_v / d xi_a of the trilinear shape functions at the tensor points."""
    dtype = np.dtype(dtype).type
    p = np.asarray(pts, dtype=dtype)
    n = p.size
    X, Y, Z = (a.reshape(-1) for a in np.meshgrid(p, p, p, indexing="ij"))
    out = np.zeros((3, n**3, 8), dtype=dtype)
    one = dtype(1)
    for v in range(8):
        vx, vy, vz = v & 1, (v >> 1) & 1, (v >> 2) & 1
        lx, ly, lz = (X if vx else one - X), (Y if vy else one - Y), (Z if vz else one - Z)
        dx, dy, dz = (one if vx else -one), (one if vy else -one), (one if vz else -one)
        out[0, :, v] = dx * ly * lz
        out[1, :, v] = lx * dy * lz
        out[2, :, v] = lx * ly * dz
    return out


def jacobians(x_dofs, x_g, pts, dtype=np.float64):
    """``J_[c, q, a, d] = sum_v dN_v/dxi_a(q) X[c, v, d]``."""
    X = np.asarray(x_g, dtype=dtype)[np.asarray(x_dofs)]  # [ncell, 8, 3]
    return np.einsum("aqv,cvd->cqad", p1_gradients(pts, dtype), X)


def point_factors(x_dofs, x_g, pts, wts, dtype=np.float64):
    """``(inv(J_) [c, q, d, a], w |det| [c, q], det [c, q])``."""
    J = jacobians(x_dofs, x_g, pts, dtype)
    det = _det3(J)
    inv = _inv3(J, det)
    w = np.asarray(wts, dtype=dtype)
    w3 = (w[:, None, None] * w[None, :, None] * w[None, None, :]).reshape(-1)
    return inv, w3[None, :] * np.abs(det), det


def _det3(J):
    return (J[..., 0, 0] * (J[..., 1, 1] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 1])
            - J[..., 0, 1] * (J[..., 1, 0] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 0])
            + J[..., 0, 2] * (J[..., 1, 0] * J[..., 2, 1] - J[..., 1, 1] * J[..., 2, 0]))


def _inv3(J, det):
    """Adjugate over determinant, in the dtype of ``J``."""
    A = np.empty_like(J)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != j]
            c = [k for k in range(3) if k != i]
            minor = J[..., r[0], c[0]] * J[..., r[1], c[1]] - J[..., r[0], c[1]] * J[..., r[1], c[0]]
            A[..., i, j] = (-1) ** (i + j) * minor
    return A / det[..., None, None]


def reference_gradient(u_cells, dphi, dtype=np.float64):
    """``[c, q, a]``: du/dxi_a at the tensor points from the cell values ``u_cells [c, n^3]`` (local dof ix n^2 + iy n + iz)."""
    D = np.asarray(dphi, dtype=dtype)
    n = int(round(D.size ** 0.5))
    D = D.reshape(n, n)
    U = np.asarray(u_cells, dtype=dtype).reshape(-1, n, n, n)
    g = np.stack([np.einsum("qi,cijk->cqjk", D, U), np.einsum("qj,cijk->ciqk", D, U), np.einsum("qk,cijk->cijq", D, U)], axis=-1)
    return g.reshape(U.shape[0], n**3, 3)


def weighted_gradient(x_dofs, x_g, pts, wts, dphi, dofmap, u, dtype=np.float64):
    """``r[c, q, d] = w |det| (inv(J_) grad_xi u)_d`` per cell and point."""
    inv, wdet, _ = point_factors(x_dofs, x_g, pts, wts, dtype)
    gh = reference_gradient(np.asarray(u, dtype=dtype)[np.asarray(dofmap)], dphi, dtype)
    return wdet[..., None] * np.einsum("cqda,cqa->cqd", inv, gh)


def scatter3(r, cell_constants, dofmap, ndofs, y3=None):
    """``y3[d, dofmap[c, q]] += c_c r[c, q, d]``; returns y3 (``[3, ndofs]``, dtype of r unless given)."""
    y3 = np.zeros((3, ndofs), dtype=r.dtype) if y3 is None else y3
    dm = np.asarray(dofmap).reshape(-1)
    cr = np.asarray(cell_constants, dtype=r.dtype)[:, None, None] * r
    for d in range(3):
        np.add.at(y3[d], dm, cr[..., d].reshape(-1))
    return y3


def weak_gradient(x_dofs, x_g, pts, wts, dphi, dofmap, u, cell_constants, ndofs, y3=None, dtype=np.float64):
    """The operator: ``y3 += C(c) u``."""
    return scatter3(weighted_gradient(x_dofs, x_g, pts, wts, dphi, dofmap, u, dtype), cell_constants, dofmap, ndofs, y3)


def lumped_mass(x_dofs, x_g, pts, wts, dofmap, cell_constants, ndofs):
    """``M(c) 1``."""
    _, wdet, _ = point_factors(x_dofs, x_g, pts, wts)
    out = np.zeros(ndofs)
    np.add.at(out, np.asarray(dofmap).reshape(-1), (np.asarray(cell_constants, dtype=np.float64)[:, None] * wdet).reshape(-1))
    return out


class Geometry:
    """What the maps share: the mesh pair, the 1-D tables and the dofmap."""

    def __init__(self, x_dofs, x_g, pts, wts, dphi, dofmap, ndofs):
        self.x_dofs, self.x_g, self.pts, self.wts, self.dphi, self.dofmap, self.ndofs = x_dofs, x_g, pts, wts, dphi, dofmap, int(ndofs)
        self.vol = lumped_mass(x_dofs, x_g, pts, wts, dofmap, np.ones(np.asarray(dofmap).shape[0]), ndofs)

    @classmethod
    def of_mesh(cls, mesh, pts, wts, dphi):
        return cls(mesh.x_dofs, mesh.x_g, pts, wts, dphi, mesh.dofmap, mesh.ndofs)

    def mass(self, cell_constants):
        return lumped_mass(self.x_dofs, self.x_g, self.pts, self.wts, self.dofmap, cell_constants, self.ndofs)


def recovered_gradient(geo, field, cell_constants=None):
    """``C(c) field / M(1) 1``, ``[3, ndofs]``."""
    c = np.ones(np.asarray(geo.dofmap).shape[0]) if cell_constants is None else cell_constants
    return weak_gradient(geo.x_dofs, geo.x_g, geo.pts, geo.wts, geo.dphi, geo.dofmap, field, c, geo.ndofs) / geo.vol


def intensity_of(geo, k, omega, re, im, rho_cells):
    """``(Im P g(Re P) - Re P g(Im P)) / (2 k w)``, g the recovered gradient with cell constant 1 / rho."""
    rinv = 1.0 / np.asarray(rho_cells, dtype=np.float64)
    return (im * recovered_gradient(geo, re, rinv) - re * recovered_gradient(geo, im, rinv)) / (2.0 * k * omega)


def particle_velocity(geo, k, omega, re, im, rho_cells):
    """``V = i grad(P) / (k w rho)`` -> (re, im)."""
    rinv = 1.0 / np.asarray(rho_cells, dtype=np.float64)
    return -recovered_gradient(geo, im, rinv) / (k * omega), recovered_gradient(geo, re, rinv) / (k * omega)


def radiation_force(geo, harmonics, delta_cells, rho_cells, c_cells):
    """``sum_k (M(2 alpha_k / c) 1 / M(1) 1) I_k``, ``alpha_k = delta (k w)^2 / (2 c^3)``; ``harmonics``: (k, omega, re, im) each."""
    delta, c = np.asarray(delta_cells, dtype=np.float64), np.asarray(c_cells, dtype=np.float64)
    total = np.zeros((3, geo.ndofs))
    for k, omega, re, im in harmonics:
        total += geo.mass(delta * (k * omega) ** 2 / c**4) / geo.vol * intensity_of(geo, k, omega, re, im, rho_cells)
    return total
