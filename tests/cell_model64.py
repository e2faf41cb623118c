"""An fp64 model of the constant-coefficient cell operators on inputs rounded to the kernel's type ONCE, for
tests/test_cell_builds_gpu.py (built as tests/nodal_model64.py is for the two nodal kernels):

    general      y += K(cc) x                                        stiffness_plan_kernel, stiffness_plan_rows_kernel
    affine       y += K(cc) x,  G[c, q] = G[c, 0] w_q / w_0          stiffness_plan_affine_kernel
    geom         y += K(cc) x,  G formed from the cell vertices      stiffness_plan_geom_kernel
    westervelt   b += K(c3) u + K(c4) v + M(c5) v^2,  m += M(c2) u   westervelt_cell_kernel       (MASS; without: b += K(c3) u + K(c4) v)
    westervelt_geom   the same, G and detJ from the cell vertices    westervelt_cell_geom_kernel

and, for tests/test_cell_op_builds_gpu.py,

    mass         y += M(c) x on cells, detJ read from its array      mass_plan_kernel, mass_kernel
    facet_mass   the same on boundary facets, N = n^2                mass_plan_kernel, mass_kernel
    gradient     y3 += C(c) x, the geometry from the cell vertices   gradient_plan_geom_kernel

The model reads what each kernel reads.  General G: ``G`` and ``detJ`` of ``build_problem(dtype=T)`` cast to float64 -- not
re-formed from the vertices.  Affine: ``f64(G_T[c, 0, :]) * f64(wratio_T[q])`` with ``wratio_T = (w / w[0]).astype(T)`` as
``operators._StiffnessOperator`` builds it, on an unperturbed box that a fixed linear map shears (the cells stay affine, all six
components of G are non-zero and differ).  In-kernel geometry: ``nodal_model64.factors64`` and the fp64 ``detJ`` of the same rounded
vertices and tables.  The apply is ``oracle_c.stiffness_apply`` / ``mass_apply`` on float64 arrays.

A case holds its inputs in the case's type and one record per output vector under ``case["out"]``: ``y`` for the three stiffness
kinds; ``b`` and ``m`` (the full pass) and ``bs`` (the stiffness part alone) for the two Westervelt kinds.  A record is what
``nodal_model64._finish`` makes: ``y0``, ``add``, ``ref`` = y0 + add in float64 and, for fp32, ``cpu32`` / ``e_cpu``: the fp32 CPU
oracle (the same calls on the type-T arrays; v^2 rounded once) on top of the same y0 and its distance (rel l2, rel max) from the model.

Inputs are seeded per (kind, degree, type).  x / u / v are independent standard normals.  The four Westervelt constants lie on ranges
that do not meet, so that any swap among them is an O(1) error: c3 is the geometry's ``cc`` (around 1), c4 on [-1.5, -0.5], c2 on
[0.2, 0.4], c5 = s x [2, 3] with s = rms(K(c3) u + K(c4) v) / rms(M(1) v^2), a power of two, so that the mass term of ``b`` is as large
as its stiffness terms (on a unit box detJ is orders of magnitude below the entries of K; with c5 = O(1) a wrong c5 would vanish in
``b``).  y0 / b0 / m0 are Gaussian at 0.1 x the rms of what is added.  Cases are read-only.  CPU only.  Not a test module; what the
GPU tests take for granted about it is checked in tests/test_cell_model64.py.

The two mass kinds read ``dofmap`` [entities, N], ``detJ`` of the same shape and ``cc`` (one constant per entity) of any geometry that
holds them (``box``, ``colliding``, ``facet_box``, ``entities``); the apply is ``oracle_c.mass_apply``.  The gradient kind is
``gradient_cpu.weak_gradient`` in float64 on the rounded vertices and tables, with one record per component (``gx``, ``gy``, ``gz``);
its fp32 evaluation is the same function with ``dtype=np.float32``, whose einsum order is not the kernel's and whose rel max error
reaches several units of 2^-23 on thin boxes: every record carries ``e_bar``, the e_cpu that enters the fp32 bar, which for the
gradient is e_cpu capped at ``E_CAP`` = 2 units (the bound the other kinds meet) and for every other kind e_cpu itself."""

import numpy as np

import gradient_cpu
import nodal_model64 as nodal
from conftest import build_problem, pkg

KINDS = {"general": 3, "affine": 4, "geom": 5, "westervelt": 6, "westervelt_geom": 7}  # (1, 2: nodal_model64's)
OP_KINDS = {"mass": 8, "facet_mass": 9, "gradient": 10}  # the kinds of tests/test_cell_op_builds_gpu.py: the ids go on, no draw above changes
E_CAP = 2 * 2.0**-23  # the cap on the gradient restatement's e_cpu in the fp32 bar
# the linear map of the affine box: det 0.83, every entry of J^-1 J^-T non-zero
SHEAR = np.array([[1.0, 0.3, -0.2], [0.1, 0.8, 0.25], [-0.15, 0.2, 1.2]])

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        from oracle.oracle_c import OracleLib

        _oracle = OracleLib()
    return _oracle


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def factors(geo, dtype):
    """(G, detJ) in ``dtype`` from the vertices and the 1-D rule of ``geo`` (both cast to ``dtype`` first), formed as
    ``build_problem`` forms them."""
    gll, pre = pkg("gll"), pkg("precompute")
    pts, wts, nq = geo["pts"].astype(dtype), geo["wts"].astype(dtype), (geo["P"] + 1) ** 3
    dphi_g = pre.tabulate_hex_p1_gradients(gll.tensor_points_3d(pts), dtype)
    wts3 = gll.tensor_weights_3d(wts).astype(dtype)
    mesh = (geo["x_dofs"], np.ascontiguousarray(geo["x_g"].astype(dtype)))
    G, detJ = np.zeros((geo["ncells"], nq, 6), dtype=dtype), np.zeros((geo["ncells"], nq), dtype=dtype)
    pre.compute_scaled_geometrical_factor(G, mesh, geo["ncells"], dphi_g, wts3)
    pre.compute_scaled_jacobian_determinant(detJ, mesh, geo["ncells"], dphi_g, wts3)
    return G, detJ


def box(P, shape, dtype, perturb=0.2, seed=None):
    """``nodal_model64.box`` and ``detJ`` of the same ``build_problem`` next to its ``G``."""
    geo = nodal.box(P, shape, dtype, perturb, seed)
    pb = build_problem(P, shape, dtype=dtype, perturb=perturb, seed=40 + P if seed is None else seed)
    assert np.array_equal(pb["G"], geo["G"])
    geo["detJ"] = pb["detJ"]
    return geo


def affine_box(P, shape, dtype):
    """An unperturbed box mapped by ``SHEAR``: every cell the same parallelepiped.  ``G`` / ``detJ`` in ``dtype`` from the mapped
    vertices rounded to ``dtype``; ``w3``: the tensor weights the operator takes as ``affine_weights``."""
    geo = box(P, shape, dtype, perturb=0.0)
    geo["x_g"] = np.ascontiguousarray((_f64(geo["x_g"]) @ SHEAR.T).astype(dtype))
    geo["G"], geo["detJ"] = factors(geo, dtype)
    geo["w3"] = pkg("gll").tensor_weights_3d(geo["wts"])
    return geo


def colliding(dtype, affine=False, P=3, ncells=37, ndofs=50, seed=3):
    """``nodal_model64.colliding`` (dofmap rows are random integers in [0, ndofs); geometry of a 2 x 2 x 2 mesh, tiled) with ``detJ``
    tiled as ``G`` is; ``affine``: the tiled geometry is that of ``affine_box`` (the draws are the same)."""
    geo = nodal.colliding(dtype, P, ncells, ndofs, seed)
    base = affine_box(P, (2, 2, 2), dtype) if affine else box(P, (2, 2, 2), dtype, perturb=0.1, seed=0)
    reps = -(-ncells // base["ncells"])
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:ncells])  # noqa: E731
    if affine:
        geo.update(x_g=base["x_g"], w3=base["w3"])
    else:
        assert np.array_equal(geo["G"], tile(base["G"]))
    geo.update(G=tile(base["G"]), detJ=tile(base["detJ"]))
    return geo


def affine_G(geo, dtype):
    """What the affine kernel makes of G, in ``dtype``: the first record of each cell times ``wratio``; and ``wratio`` in the case's type."""
    w = _f64(geo["w3"]).reshape(-1)
    wratio = (w / w[0]).astype(geo["dtype"])
    return np.ascontiguousarray(geo["G"][:, :1, :].astype(dtype) * wratio.astype(dtype)[None, :, None]), wratio


def _rng(kind, geo, salt):
    return np.random.default_rng([KINDS[kind] if kind in KINDS else OP_KINDS[kind], geo["P"], geo["dtype"].itemsize, salt])


def _freeze(case):
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _record(geo, add, rng, oracle32):
    return nodal._finish(dict(dtype=geo["dtype"], ndofs=geo["ndofs"]), {}, add, rng, oracle32)


def _geometry64(kind, geo):
    """(G, detJ) in float64 as the kernels of ``kind`` read them, and the G in the case's type that the fp32 oracle applies."""
    if kind == "affine":
        return affine_G(geo, np.float64)[0], _f64(geo["detJ"]), affine_G(geo, geo["dtype"])[0]
    if kind in ("geom", "westervelt_geom"):
        return factors(geo, np.float64) + (geo["G"],)
    return _f64(geo["G"]), _f64(geo["detJ"]), geo["G"]


def stiffness(kind, geo, salt=0):
    """One case of ``y += K(cc) x`` for ``kind`` in general / affine / geom: ``x``, ``cc``, the geometry, ``out["y"]``."""
    P, dtype, dm, nd = geo["P"], geo["dtype"], geo["dofmap"], geo["ndofs"]
    rng = _rng(kind, geo, salt)
    x = rng.standard_normal(nd).astype(dtype)
    G64, _, G32 = _geometry64(kind, geo)
    orc = oracle()
    add = np.zeros(nd)
    orc.stiffness_apply(P, _f64(geo["D"]), _f64(x), _f64(geo["cc"]), add, G64, dm)
    y = _record(geo, add, rng, lambda y: orc.stiffness_apply(P, geo["D"], x, geo["cc"], y, G32, dm))
    case = dict(geo, kind=kind, x=x, out={"y": y})
    if kind == "affine":
        case["wratio"] = affine_G(geo, dtype)[1]
    return _freeze(case)


def westervelt_add(P, D, u, v, c3, c4, G, dm, b, mass=None, m=None):
    """``b += K(c3) u + K(c4) v`` and, with ``mass = (c2, c5, detJ)``, ``b += M(c5) v^2`` (v^2 rounded to the arrays' type once) and
    ``m += M(c2) u``: the oracle's calls in the order of the four launches the fused pass replaces, in the type of the arguments."""
    orc = oracle()
    orc.stiffness_apply(P, D, u, c3, b, G, dm)
    orc.stiffness_apply(P, D, v, c4, b, G, dm)
    if mass is not None:
        c2, c5, detJ = mass
        orc.mass_apply(np.ascontiguousarray((v * v).astype(u.dtype)), c5, b, detJ, dm)
        if m is not None:
            orc.mass_apply(u, c2, m, detJ, dm)


def westervelt(kind, geo, salt=0, swap=()):
    """One case of the Westervelt cell pass for ``kind`` in westervelt / westervelt_geom: ``u``, ``v``, ``c2`` .. ``c5``, the geometry;
    ``out["b"]`` and ``out["m"]`` of the full pass, ``out["bs"]`` of the stiffness part alone; ``ks`` / ``mb``: the stiffness and the
    mass part of what is added to b.  ``swap``: pairs of constants the MODEL exchanges (("c2", "c5"), ...), for the test of the inputs."""
    P, dtype, dm, nd, nc = geo["P"], geo["dtype"], geo["dofmap"], geo["ndofs"], geo["ncells"]
    rng = _rng(kind, geo, salt)
    u, v = rng.standard_normal(nd).astype(dtype), rng.standard_normal(nd).astype(dtype)
    c3, c4 = geo["cc"], rng.uniform(-1.5, -0.5, nc).astype(dtype)
    c2, c5 = rng.uniform(0.2, 0.4, nc).astype(dtype), rng.uniform(2.0, 3.0, nc)
    G64, detJ64, G32 = _geometry64(kind, geo)
    D64, u64, v64 = _f64(geo["D"]), _f64(u), _f64(v)
    ks, mb1 = np.zeros(nd), np.zeros(nd)
    westervelt_add(P, D64, u64, v64, _f64(c3), _f64(c4), G64, dm, ks)
    oracle().mass_apply(v64 * v64, c5, mb1, detJ64, dm)
    c5 = (c5 * 2.0 ** np.round(np.log2(np.sqrt(np.mean(ks**2) / np.mean(mb1**2))))).astype(dtype)
    k = dict(c2=c2, c3=c3, c4=c4, c5=c5)
    for a, b in swap:
        k[a], k[b] = k[b], k[a]
    ks, full, mm = np.zeros(nd), np.zeros(nd), np.zeros(nd)
    westervelt_add(P, D64, u64, v64, _f64(k["c3"]), _f64(k["c4"]), G64, dm, ks)
    westervelt_add(P, D64, u64, v64, _f64(k["c3"]), _f64(k["c4"]), G64, dm, full, (_f64(k["c2"]), _f64(k["c5"]), detJ64), mm)
    mass32 = (c2, c5, geo["detJ"])
    out = {"b": _record(geo, full, rng, lambda y: westervelt_add(P, geo["D"], u, v, c3, c4, G32, dm, y, mass32)),
           "m": _record(geo, mm, rng, lambda y: oracle().mass_apply(u, c2, y, geo["detJ"], dm)),
           "bs": _record(geo, ks, rng, lambda y: westervelt_add(P, geo["D"], u, v, c3, c4, G32, dm, y))}
    return _freeze(dict(geo, kind=kind, u=u, v=v, c2=c2, c3=c3, c4=c4, c5=c5, out=out, ks=ks, mb=full - ks))


def facet_box(P, shape, dtype, perturb=0.2):
    """The boundary facets of a perturbed box as mass entities: ``dofmap`` [facets, n^2], ``detJ`` (the scaled surface determinant in
    ``dtype``, formed as the solvers form it) and ``cc``, one constant per facet around 1."""
    gll, pre = pkg("gll"), pkg("precompute")
    mesh = pkg("boxmesh").BoxMesh(P, shape, perturb=perturb, seed=40 + P, dtype=dtype)
    pts, wts, _ = gll.tabulate_1d(P, dtype)
    bd = mesh.boundary_facets()
    dF = np.zeros((bd.shape[0], (P + 1) ** 2), dtype=dtype)
    pre.compute_boundary_facets_scaled_jacobian_determinant(dF, (mesh.x_dofs, mesh.x_g), bd, pre.tabulate_facet_gradients(pts, dtype),
                                                            gll.tensor_weights_2d(wts).astype(dtype))
    cc = (1.0 + 0.25 * np.random.default_rng(77 + P).standard_normal(bd.shape[0])).astype(dtype)
    return dict(P=P, dtype=np.dtype(dtype), ndofs=mesh.ndofs, ncells=bd.shape[0], dofmap=np.ascontiguousarray(mesh.facet_dofmap(bd), dtype=np.int32),
                detJ=dF, cc=cc)


def entities(dtype, N, nent, ndofs, seed=5):
    """A synthetic entity set for the plan-free mass kernel: ``dofmap`` rows are random integers in [0, ndofs) (N = 1 included), ``detJ``
    uniform on [0.5, 1.5], ``cc`` around 1.  ``P`` is N (it only seeds the draws)."""
    rng = np.random.default_rng([seed, N, nent])
    return dict(P=N, dtype=np.dtype(dtype), ndofs=ndofs, ncells=nent, dofmap=rng.integers(0, ndofs, size=(nent, N), dtype=np.int32),
                detJ=rng.uniform(0.5, 1.5, (nent, N)).astype(dtype), cc=(1.0 + 0.25 * rng.standard_normal(nent)).astype(dtype))


def mass(kind, geo, salt=0):
    """One case of ``y += M(cc) x`` on the entities of ``geo``: ``x``, ``out["y"]``."""
    dtype, dm, nd = geo["dtype"], geo["dofmap"], geo["ndofs"]
    rng = _rng(kind, geo, salt)
    x = rng.standard_normal(nd).astype(dtype)
    orc = oracle()
    add = np.zeros(nd)
    orc.mass_apply(_f64(x), _f64(geo["cc"]), add, _f64(geo["detJ"]), dm)
    y = _record(geo, add, rng, lambda y: orc.mass_apply(x, geo["cc"], y, geo["detJ"], dm))
    y["e_bar"] = y["e_cpu"]
    return _freeze(dict(geo, kind=kind, x=x, out={"y": y}))


COMPONENTS = ("gx", "gy", "gz")


def gradient(kind, geo, salt=0):
    """One case of ``y3 += C(cc) x``: ``x`` and one record per component under ``out`` (``COMPONENTS``), each with its own y0."""
    dtype, dm, nd = geo["dtype"], geo["dofmap"], geo["ndofs"]
    rng = _rng(kind, geo, salt)
    x = rng.standard_normal(nd).astype(dtype)
    tables = (geo["x_dofs"], geo["x_g"], geo["pts"], geo["wts"], geo["D"])
    add = gradient_cpu.weak_gradient(*tables, dm, _f64(x), _f64(geo["cc"]), nd)
    out = {}
    if dtype == np.float32:  # what weak_gradient(..., y3=y0, dtype=np.float32) adds, component by component
        r32 = gradient_cpu.weighted_gradient(*tables, dm, x, np.float32)
        cr32 = geo["cc"].astype(np.float32)[:, None, None] * r32
        assert cr32.dtype == np.float32
    for d, k in enumerate(COMPONENTS):
        out[k] = _record(geo, np.ascontiguousarray(add[d]), rng, lambda y, d=d: np.add.at(y, dm.reshape(-1), cr32[..., d].reshape(-1)))
        e = out[k]["e_cpu"]
        out[k]["e_bar"] = None if e is None else (min(e[0], E_CAP), min(e[1], E_CAP))
    return _freeze(dict(geo, kind=kind, x=x, out=out))


def model(kind, geo, salt=0):
    if kind in ("mass", "facet_mass"):
        return mass(kind, geo, salt)
    if kind == "gradient":
        return gradient(kind, geo, salt)
    return (westervelt if kind.startswith("westervelt") else stiffness)(kind, geo, salt)
