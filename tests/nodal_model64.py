"""An fp64 model of the two nodal cell operators on inputs rounded to the kernel's type ONCE, for tests/test_nodal_builds_gpu.py
(as tests/test_gradient_gpu.py::_case does for the gradient operator):

    stiffness:  y = y0 + K(cc kappa) x                      (csrc/stiffness_geom_nodal.hpp)
    pair:       b = b0 + K(c3 kappa3) u + K(c4 kappa4) v    (csrc/westervelt_geom_nodal.hpp)

Every input the kernel reads -- vertices, 1-D points / weights / derivative table, vectors, coefficients, cell constants, y0 -- is
rounded to ``dtype`` and cast to float64; G is formed in float64 from those rounded vertices and tables (the package's host
``precompute``), and the apply is tests/nodal_cpu.py / tests/westervelt_nodal_cpu.py in float64.  What is left between the model and a
kernel of type ``dtype`` is the kernel's own arithmetic.

For fp32 a case also carries the fp32 CPU oracle's result on the same inputs (the same two functions on fp32 arrays and the fp32 G of
``build_problem(dtype=np.float32)``) and ``e_cpu``, its distance (rel l2, rel max) from the fp64 model: the size of an honest fp32
evaluation's error, which the fp32 bar of the GPU tests is built on.

Inputs are seeded per (operator, degree, type).  kappa is drawn independently per dof, log-uniform on [0.3, 3] (a coefficient taken from
a neighbouring dof is an O(1) error, which a smooth field would hide); c4 on [-1.5, -0.5] next to the positive ``pb["cc"]`` (a swap or
a lost sign is an O(1) error); x / u / v independent standard normals; y0 Gaussian at 0.1 x the rms of what the apply adds (large
enough to be missed if overwritten, too small to hide an error).  Cases are read-only.  CPU only.  Not a test module; what the GPU
tests take for granted about it is checked in tests/test_nodal_model64.py."""

import numpy as np

import nodal_cpu
import westervelt_nodal_cpu
from conftest import build_problem, pkg, rel_l2, rel_max

_KINDS = {"stiffness": 1, "pair": 2}


def box(P, shape, dtype, perturb=0.2, seed=None):
    """The geometry of a perturbed (non-affine) box, as ``build_problem(P, shape, dtype, perturb, seed=40 + P)``: what both operators
    take besides their vectors.  ``G`` is the factor array in ``dtype`` (read by the fp32 oracle only)."""
    pb = build_problem(P, shape, dtype=dtype, perturb=perturb, seed=40 + P if seed is None else seed)
    mesh = pb["mesh"]
    return dict(P=P, dtype=np.dtype(dtype), ndofs=mesh.ndofs, ncells=mesh.ncells, dofmap=mesh.dofmap, x_dofs=mesh.x_dofs,
                x_g=np.ascontiguousarray(mesh.x_g.astype(dtype)), pts=pb["pts"], wts=pb["wts"], D=pb["D"], cc=pb["cc"], G=pb["G"])


def colliding(dtype, P=3, ncells=37, ndofs=50, seed=3):
    """Scatter-add under heavy collisions (tests/test_operators_gpu.py::test_colliding_dofmap): dofmap rows are random integers in
    [0, ndofs); ``x_dofs`` and the geometry are those of a perturbed 2 x 2 x 2 mesh, tiled."""
    geo = box(P, (2, 2, 2), dtype, perturb=0.1, seed=0)
    rng = np.random.default_rng(seed)
    reps = -(-ncells // geo["ncells"])
    geo.update(ndofs=ndofs, ncells=ncells, dofmap=rng.integers(0, ndofs, size=(ncells, (P + 1) ** 3), dtype=np.int32),
               x_dofs=np.ascontiguousarray(np.tile(geo["x_dofs"], (reps, 1))[:ncells]),
               G=np.ascontiguousarray(np.tile(geo["G"], (reps, 1, 1))[:ncells]), cc=rng.standard_normal(ncells).astype(dtype))
    return geo


def factors64(geo):
    """G in float64 from the vertices and the 1-D rule as the kernel reads them (rounded to the case's type)."""
    gll, pre = pkg("gll"), pkg("precompute")
    pts, wts = geo["pts"].astype(np.float64), geo["wts"].astype(np.float64)
    dphi_g = pre.tabulate_hex_p1_gradients(gll.tensor_points_3d(pts), np.float64)
    G = np.zeros((geo["ncells"], (geo["P"] + 1) ** 3, 6))
    pre.compute_scaled_geometrical_factor(G, (geo["x_dofs"], geo["x_g"].astype(np.float64)), geo["ncells"], dphi_g, gll.tensor_weights_3d(wts))
    return G


def _rng(kind, geo, salt):
    return np.random.default_rng([_KINDS[kind], geo["P"], geo["dtype"].itemsize, salt])


def _log_uniform(rng, size, dtype, lo=0.3, hi=3.0):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size)).astype(dtype)


def _finish(geo, case, add, rng, oracle32):
    """y0, the reference ``y0 + add`` in float64, and (fp32) the oracle's result on top of the same y0 with its distance."""
    dtype = geo["dtype"]
    y0 = (0.1 * np.sqrt(np.mean(add**2)) * rng.standard_normal(geo["ndofs"])).astype(dtype)
    ref = y0.astype(np.float64) + add
    case.update(geo, y0=y0, add=add, ref=ref, cpu32=None, e_cpu=None)
    if dtype == np.float32:
        y32 = y0.copy()
        oracle32(y32)
        assert y32.dtype == np.float32
        case.update(cpu32=y32, e_cpu=(rel_l2(y32, ref), rel_max(y32, ref)))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def stiffness(geo, salt=0):
    """One case of ``y += K(cc kappa) x``: the inputs (``x``, ``kappa``, ``cc``, ``y0`` in the case's type), ``add`` = K(cc kappa) x and
    ``ref`` = y0 + add in float64, ``cpu32`` / ``e_cpu`` for fp32."""
    P, dtype, dm, nd = geo["P"], geo["dtype"], geo["dofmap"], geo["ndofs"]
    rng = _rng("stiffness", geo, salt)
    x = rng.standard_normal(nd).astype(dtype)
    kappa = _log_uniform(rng, nd, dtype)
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    add = np.zeros(nd)
    nodal_cpu.stiffness_apply(P, f64(geo["D"]), f64(x), f64(geo["cc"]), add, factors64(geo), dm, f64(kappa))
    return _finish(geo, dict(kind="stiffness", x=x, kappa=kappa), add, rng,
                   lambda y: nodal_cpu.stiffness_apply(P, geo["D"], x, geo["cc"], y, geo["G"], dm, kappa))


def pair(geo, salt=0):
    """One case of ``b += K(c3 kappa3) u + K(c4 kappa4) v``: ``u``, ``v``, ``k3``, ``k4``, ``c3`` (= the geometry's ``cc``), ``c4``,
    ``y0``; ``add``, ``ref``, ``cpu32`` / ``e_cpu`` as ``stiffness``."""
    P, dtype, dm, nd = geo["P"], geo["dtype"], geo["dofmap"], geo["ndofs"]
    rng = _rng("pair", geo, salt)
    u, v = rng.standard_normal(nd).astype(dtype), rng.standard_normal(nd).astype(dtype)
    k3, k4 = _log_uniform(rng, nd, dtype), _log_uniform(rng, nd, dtype)
    c3, c4 = geo["cc"], rng.uniform(-1.5, -0.5, geo["ncells"]).astype(dtype)
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    add = np.zeros(nd)
    westervelt_nodal_cpu.stiffness_pair(P, f64(geo["D"]), f64(u), f64(v), f64(c3), f64(c4), add, factors64(geo), dm, f64(k3), f64(k4))
    return _finish(geo, dict(kind="pair", u=u, v=v, k3=k3, k4=k4, c3=c3, c4=c4), add, rng,
                   lambda b: westervelt_nodal_cpu.stiffness_pair(P, geo["D"], u, v, c3, c4, b, geo["G"], dm, k3, k4))


MODELS = {"stiffness": stiffness, "pair": pair}
