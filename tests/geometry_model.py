"""A model of the device geometry precompute (csrc/geometry.hpp: geometry_kernel, facet_geometry_kernel) for
tests/test_small_kernels_gpu.py, built as tests/cell_model64.py is for the cell kernels.

    J_[a][d]   = sum_v dphi[a][q][v] x[v][d]
    G[c, q, :] = |det| w / det^2 * (A^T A), A the closed-form adjugate (A[d][a] / det = inv(J_)[d][a]), upper triangle 00 01 02 11 12 22
    detJ[c, q] = |det| w
    detJ_f     = |J_[a0] x J_[a1]| w, (a0, a1) = FACET_AXES[local facet]

``model`` / ``facet_model`` evaluate that in ``numpy.longdouble`` on inputs rounded ONCE to the kernel's type T (fp64 numpy carries the
very error that is to be measured in an fp64 kernel).  ``restate`` / ``facet_restate`` are the kernel in T itself: its operation order,
no FMA.  Their distance from the model is ``e_cpu``; the GPU tests hold the kernel to 8 x e_cpu.

Errors are per (cell, q): max_k |dG_k| / ||G(c, q)||_F (the off-diagonal entries counted twice in the norm) and |d detJ| / detJ; ``errors``
returns the maximum and the root mean square over a case.  Off-diagonal entries pass through zero: no per-entry relative error.

Cells (``cells``): the unit cube mapped by I + S (S: zero diagonal, off-diagonal entries uniform in [-0.4, 0.4]), every vertex moved by
0.3 x uniform[-0.5, 0.5] (at most 0.15 h), the cell translated by up to TRANSLATION = 2 h per axis, all scaled by h; every second cell mirrored in x
(negative determinant); vertices numbered through a random permutation, so that ``x_dofs`` is neither monotone nor block-wise.  The
FAMILIES switch these on one by one, so that an error confined to one of them shows in the families that have it and in no other:

    aligned          boxes with edges in [0.6, 1.4], translated: no shear, no vertex move, no mirrored cell
    sheared          I + S, vertices moved, translated: no mirrored cell
    mirrored         the same with every second cell mirrored, h = 1
    mirrored_1e-3    ... h = 1e-3
    mirrored_1e-4    ... h = 1e-4

The quadrature (``rule`` / ``facet_rule``) is random points of the unit cube (of each of its six faces) that include corners, with
random weights in [0.1, 1.1]; ``dphi`` comes from ``precompute.tabulate_hex_p1_gradients``.  CPU only; not a test module: what the GPU
tests take for granted about it is checked in tests/test_geometry_model.py."""

import numpy as np

from conftest import pkg

LD = np.longdouble
FAMILIES = {"aligned": dict(h=1.0, shear=False, mirror=False), "sheared": dict(h=1.0, shear=True, mirror=False),
            "mirrored": dict(h=1.0, shear=True, mirror=True), "mirrored_1e-3": dict(h=1e-3, shear=True, mirror=True),
            "mirrored_1e-4": dict(h=1e-4, shear=True, mirror=True)}
NQ = (1, 7, 27, 1331)
NQF = (1, 4, 9, 121)
FACET_AXES = ((0, 1), (0, 2), (1, 2), (1, 2), (0, 2), (0, 1))  # kFacetAxes of csrc/geometry.hpp
UNIT = {np.dtype(np.float32): 2.0**-24, np.dtype(np.float64): 2.0**-53}
E_CPU_CAP = 32  # units: a condition on the inputs (they are well conditioned), not a measurement
BAR = 8  # x e_cpu: the bar of tests/test_cell_builds_gpu.py
# cells lie up to this many h from the origin, per axis.  The translation is what the restatement's error comes from (J_ is a difference of
# coordinates): at 5 h the fp64 detJ of the sheared family reached 42.9 units over 40 cells x 1331 points, above the cap; at 2 h every
# family stays below it
TRANSLATION = 2.0
PERIOD = 997  # the sweep cases repeat the geometry of this many cells

_CORNERS = np.array([[v & 1, (v >> 1) & 1, (v >> 2) & 1] for v in range(8)], dtype=np.float64)


def cell_coordinates(family, ncell, seed=0):
    """float64 [ncell, 8, 3]: the vertices of ``ncell`` cells of ``family``, vertex v = vx + 2 vy + 4 vz."""
    f = FAMILIES[family]
    rng = np.random.default_rng([11, list(FAMILIES).index(family), seed])
    if f["shear"]:
        M = np.tile(np.eye(3), (ncell, 1, 1))
        S = rng.uniform(-0.4, 0.4, (ncell, 3, 3))
        S[:, [0, 1, 2], [0, 1, 2]] = 0.0
        M += S
        X = np.einsum("cde,ve->cvd", M, _CORNERS) + 0.3 * rng.uniform(-0.5, 0.5, (ncell, 8, 3))
    else:
        X = _CORNERS[None] * rng.uniform(0.6, 1.4, (ncell, 1, 3))
    X = X + rng.uniform(-TRANSLATION, TRANSLATION, (ncell, 1, 3))
    if f["mirror"]:
        X[1::2, :, 0] *= -1.0
    return X * f["h"]


def cells(family, ncell, dtype, seed=0, period=None):
    """(x_dofs int32 [ncell, 8], x_g T [8 ncell, 3]).  ``period``: cell c has the geometry of cell c mod period, on vertices of its own."""
    base = cell_coordinates(family, ncell if period is None else min(period, ncell), seed)
    X = base if period is None else base[np.arange(ncell) % base.shape[0]]
    perm = np.random.default_rng([12, seed, ncell]).permutation(8 * ncell)
    x_g = np.empty((8 * ncell, 3), dtype=dtype)
    x_g[perm] = X.reshape(-1, 3).astype(dtype)
    return np.ascontiguousarray(perm.reshape(ncell, 8).astype(np.int32)), x_g


def _points(rng, nq, dim):
    """``nq`` points of the unit ``dim``-cube: min(nq // 2, 2^dim) of its corners (drawn without repeat), the others uniform."""
    k = min(nq // 2, 2**dim)
    corners = _CORNERS[: 2**dim, :dim][rng.permutation(2**dim)[:k]]
    return np.concatenate([corners, rng.random((nq - k, dim))])[rng.permutation(nq)]


def rule(nq, dtype, seed=0):
    """(dphi T [3, nq, 8], weights T [nq])."""
    rng = np.random.default_rng([13, nq, seed])
    pts = _points(rng, nq, 3)
    return pkg("precompute").tabulate_hex_p1_gradients(pts, dtype), rng.uniform(0.1, 1.1, nq).astype(dtype)


def facet_rule(nqf, dtype, seed=0):
    """(dphi_f T [6, 3, nqf, 8], weights T [nqf]): per local facet its own random points, embedded as ``precompute.facet_points`` does."""
    pre = pkg("precompute")
    rng = np.random.default_rng([14, nqf, seed])
    out = []
    for axis, side in pre.HEX_FACET_AXIS_SIDE:
        p2 = _points(rng, nqf, 2)
        pts = np.full((nqf, 3), float(side))
        pts[:, [a for a in range(3) if a != axis]] = p2
        out.append(pre.tabulate_hex_p1_gradients(pts, dtype))
    return np.stack(out), rng.uniform(0.1, 1.1, nqf).astype(dtype)


def boundary(ncell, nfacets, seed=0):
    """int32 [nfacets, 2]: random (cell, local facet) pairs, unsorted, cells repeat, the first six rows hold the six local facets."""
    rng = np.random.default_rng([15, ncell, nfacets, seed])
    bd = np.stack([rng.integers(0, ncell, nfacets), rng.integers(0, 6, nfacets)], axis=1).astype(np.int32)
    bd[: min(6, nfacets), 1] = np.arange(6)[: min(6, nfacets)]
    return bd


# ---- the model: longdouble on the rounded inputs --------------------------------------------------------------------------------------
def _adjugate(J):
    A = np.empty_like(J)
    A[..., 0, 0] = J[..., 1, 1] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 1]
    A[..., 0, 1] = J[..., 0, 2] * J[..., 2, 1] - J[..., 0, 1] * J[..., 2, 2]
    A[..., 0, 2] = J[..., 0, 1] * J[..., 1, 2] - J[..., 0, 2] * J[..., 1, 1]
    A[..., 1, 0] = J[..., 1, 2] * J[..., 2, 0] - J[..., 1, 0] * J[..., 2, 2]
    A[..., 1, 1] = J[..., 0, 0] * J[..., 2, 2] - J[..., 0, 2] * J[..., 2, 0]
    A[..., 1, 2] = J[..., 0, 2] * J[..., 1, 0] - J[..., 0, 0] * J[..., 1, 2]
    A[..., 2, 0] = J[..., 1, 0] * J[..., 2, 1] - J[..., 1, 1] * J[..., 2, 0]
    A[..., 2, 1] = J[..., 0, 1] * J[..., 2, 0] - J[..., 0, 0] * J[..., 2, 1]
    A[..., 2, 2] = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
    return A


def _jacobians(coords, dphi, ftype):
    """J_[c, q, a, d] in ``ftype``, accumulated over v = 0 .. 7 in turn (the kernel's order; a product and an add, no FMA)."""
    X, d = coords.astype(ftype), dphi.astype(ftype)
    J = np.zeros((X.shape[0], d.shape[1], 3, 3), dtype=ftype)
    for v in range(8):
        J += d[None, :, :, v].transpose(0, 2, 1)[..., None] * X[:, None, None, v, :]
    return J


def _factors(J, w):
    """(G [.., 6], detJ) from J_ and the weights, in J's type, in the kernel's operation order."""
    A = _adjugate(J)
    det = (J[..., 0, 0] * A[..., 0, 0] + J[..., 0, 1] * A[..., 1, 0]) + J[..., 0, 2] * A[..., 2, 0]
    sdet = np.abs(det) * w
    s = sdet / (det * det)
    G = np.empty(J.shape[:-2] + (6,), dtype=J.dtype)
    k = 0
    for a in range(3):
        for b in range(a, 3):
            G[..., k] = s * ((A[..., 0, a] * A[..., 0, b] + A[..., 1, a] * A[..., 1, b]) + A[..., 2, a] * A[..., 2, b])
            k += 1
    return G, sdet


def _evaluate(x_dofs, x_g, dphi, weights, ftype):
    G, d = _factors(_jacobians(x_g[x_dofs], dphi, ftype), weights.astype(ftype)[None, :])
    assert G.dtype == ftype and d.dtype == ftype
    return G, d


def model(x_dofs, x_g, dphi, weights):
    """(G [ncell, nq, 6], detJ [ncell, nq]) in longdouble."""
    return _evaluate(x_dofs, x_g, dphi, weights, LD)


def restate(x_dofs, x_g, dphi, weights):
    """The kernel in the type of ``x_g``."""
    return _evaluate(x_dofs, x_g, dphi, weights, x_g.dtype.type)


def _facet_evaluate(x_dofs, x_g, bd, dphi_f, weights, ftype):
    out = np.empty((bd.shape[0], weights.size), dtype=ftype)
    w = weights.astype(ftype)[None, :]
    for lf in range(6):
        sel = np.nonzero(bd[:, 1] == lf)[0]
        if sel.size == 0:
            continue
        J = _jacobians(x_g[x_dofs[bd[sel, 0]]], dphi_f[lf], ftype)
        r0, r1 = J[..., FACET_AXES[lf][0], :], J[..., FACET_AXES[lf][1], :]
        cx = r0[..., 1] * r1[..., 2] - r0[..., 2] * r1[..., 1]
        cy = r0[..., 2] * r1[..., 0] - r0[..., 0] * r1[..., 2]
        cz = r0[..., 0] * r1[..., 1] - r0[..., 1] * r1[..., 0]
        out[sel] = np.sqrt((cx * cx + cy * cy) + cz * cz) * w
    return out


def facet_model(x_dofs, x_g, bd, dphi_f, weights):
    """detJ_f [nfacets, nqf] in longdouble."""
    return _facet_evaluate(x_dofs, x_g, bd, dphi_f, weights, LD)


def facet_restate(x_dofs, x_g, bd, dphi_f, weights):
    return _facet_evaluate(x_dofs, x_g, bd, dphi_f, weights, x_g.dtype.type)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def _max_rms(e):
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    return (float(e.max()), float(np.sqrt(np.mean(e * e)))) if e.size else (0.0, 0.0)


def g_errors(G, G_model):
    """(max, rms) over (cell, q) of max_k |dG_k| / ||G(c, q)||_F."""
    Gm = np.asarray(G_model, dtype=LD)
    norm = np.sqrt(np.sum(Gm * Gm * np.array([1, 2, 2, 1, 2, 1], dtype=LD), axis=-1))
    return _max_rms(np.max(np.abs(np.asarray(G).astype(LD) - Gm), axis=-1) / norm)


def det_errors(d, d_model):
    """(max, rms) over the entries of |d - model| / model (detJ and detJ_f are positive)."""
    dm = np.asarray(d_model, dtype=LD)
    return _max_rms(np.abs(np.asarray(d).astype(LD) - dm) / dm)
