"""The sponge layer's part of the CPU wave model (``oracle/rk4_oracle.py``) for the tests: the term the layer puts into the right-hand
side of every stage,

    b -= cv * vn + cu * un,        cv = 2 sigma m,  cu = sigma^2 m        (m: the lumped mass; the Westervelt loop's m0)

before ``b / m``, as a ``stage_term`` of ``rk4_oracle.solve`` / ``solve_westervelt``: the geometry, the coefficients, the right-hand
side and the time loop are the oracle's own.  With sigma == 0 the term changes no bit (tests/test_sponge.py).  The factors of the
two coefficients are arguments (the wrong forms the constant-sigma identity must tell apart).  One rank.  Not a test module."""

import numpy as np


def _sigma(mesh, sigma):
    """sigma as one value per dof of the (single-rank) mesh: None, a scalar, an array, or a callable of the dof coordinates."""
    if sigma is None:
        return np.zeros(mesh.ndofs)
    if callable(sigma):
        return np.asarray(sigma(mesh.dof_coordinates()), dtype=np.float64)
    return np.broadcast_to(np.asarray(sigma, dtype=np.float64), (mesh.ndofs,)).copy()


def layer_term(mesh, sigma, cv_factor=2.0, cu_factor=1.0):
    """The layer as the model's ``stage_term``: given the lumped mass it returns the in-place update of a stage's ``b``."""
    sig = _sigma(mesh, sigma)

    def bind(m):
        cv, cu = cv_factor * sig * m, cu_factor * (sig * sig) * m

        def term(b, un, vn):
            b -= cv * vn + cu * un

        return term

    return bind
