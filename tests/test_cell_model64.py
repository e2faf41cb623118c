"""The fp64 model of the constant-coefficient cell operators (tests/cell_model64.py) on the CPU: what tests/test_cell_builds_gpu.py takes
for granted about its reference and about the fp32 bar built on it -- and that its build matrix names every instantiation of these
kernels that the library compiles, each once, and none that it does not (from the kernel names of a device-only compile: no GPU)."""

import os
import re
import shutil
import sys

import numpy as np
import pytest

import cell_model64 as model
import test_cell_builds_gpu as builds
from conftest import TOL, ROOT, rel_l2, rel_max

U = 2.0**-23
SHAPES = builds.SHAPES
EDGE_SHAPES = [(1, (1, 1, 1)), (4, (1, 1, 1)), (10, (1, 1, 1)), (4, (5, 2, 2)), (7, (3, 2, 2))]
STIFFNESS, WESTERVELT = ("general", "affine", "geom"), ("westervelt", "westervelt_geom")


def _geo(kind, P, shape, dtype):
    return (model.affine_box if kind == "affine" else model.box)(P, shape, dtype)


@pytest.fixture(scope="module")
def cases32():
    """The fp32 model of every kind at every degree on the shapes of the build matrix, built once."""
    return {(kind, P): model.model(kind, _geo(kind, P, SHAPES[P], np.float32)) for kind in model.KINDS for P in sorted(SHAPES)}


def test_the_cases_are_frozen(cases32):
    for c in (cases32["general", 3], cases32["affine", 4], cases32["westervelt_geom", 2]):
        arrays = [a for a in c.values() if isinstance(a, np.ndarray)] + [a for r in c["out"].values() for a in r.values() if isinstance(a, np.ndarray)]
        assert len(arrays) > 12 and not any(a.flags.writeable for a in arrays)
        for r in c["out"].values():
            assert r["ref"].dtype == np.float64 and r["y0"].dtype == r["cpu32"].dtype == np.float32
            with pytest.raises(ValueError):
                r["ref"][0] = 0.0


def test_the_geometry_model_is_that_of_the_nodal_kernels():
    """``factors`` in float64 on vertices rounded to fp32 gives the G of ``nodal_model64.factors64``; in the case's own type it gives
    ``build_problem``'s G and detJ."""
    import nodal_model64 as nodal

    geo = model.box(3, SHAPES[3], np.float32)
    assert np.array_equal(model.factors(geo, np.float64)[0], nodal.factors64(geo))
    G, detJ = model.factors(geo, np.float32)
    assert np.array_equal(G, geo["G"]) and np.array_equal(detJ, geo["detJ"]) and G.dtype == np.float32


@pytest.mark.parametrize("P", sorted(SHAPES))
def test_the_inputs_tell_the_constants_apart(cases32, P):
    """x / u / v independent; c3 around 1, c4 negative, c2 on [0.2, 0.4], c5 far above all of them and such that the mass term of b is of
    the size of its stiffness terms; y0 a tenth of what is added, for every output."""
    for kind in WESTERVELT:
        c = cases32[kind, P]
        assert rel_l2(c["u"], c["v"]) > 0.5
        assert c["c3"].min() > 0 and -1.5 <= c["c4"].min() and c["c4"].max() <= -0.5 and 0.2 <= c["c2"].min() and c["c2"].max() <= 0.4 * (1 + 1e-6)
        assert c["c5"].min() > 4 * max(c["c3"].max(), c["c2"].max()) and c["c5"].max() < 1.5 * (1 + 1e-6) * c["c5"].min()
        assert 0.25 < np.linalg.norm(c["mb"]) / np.linalg.norm(c["ks"]) < 4.0
    for kind in model.KINDS:
        for k, r in cases32[kind, P]["out"].items():
            ratio = np.sqrt(np.mean(r["y0"].astype(np.float64) ** 2) / np.mean(r["add"] ** 2))
            assert 0.08 < ratio < 0.12, (kind, k, ratio)


@pytest.mark.parametrize("kind", WESTERVELT)
@pytest.mark.parametrize("P", [1, 4, 7, 10])
def test_a_swap_of_two_constants_is_an_error_of_order_one(cases32, kind, P):
    """c2 <-> c5 or c3 <-> c4 in the MODEL moves every output that reads one of the two by more than 0.1 in rel l2."""
    c = cases32[kind, P]
    geo = _geo(kind, P, SHAPES[P], np.float32)
    s25, s34 = model.westervelt(kind, geo, swap=(("c2", "c5"),)), model.westervelt(kind, geo, swap=(("c3", "c4"),))
    for k in ("u", "v", "c2", "c3", "c4", "c5"):
        assert np.array_equal(s25[k], c[k]) and np.array_equal(s34[k], c[k])
    add = lambda case, k: case["out"][k]["add"]  # noqa: E731
    assert rel_l2(add(s25, "b"), add(c, "b")) > 0.1 and rel_l2(add(s25, "m"), add(c, "m")) > 0.1
    assert rel_l2(add(s34, "b"), add(c, "b")) > 0.1 and rel_l2(add(s34, "bs"), add(c, "bs")) > 0.1
    assert np.array_equal(add(s25, "bs"), add(c, "bs")) and np.array_equal(add(s34, "m"), add(c, "m"))


@pytest.mark.parametrize("P", [1, 3, 4, 5, 10])
def test_the_fp64_model_is_the_plain_oracle(oracle_c, P):
    """In fp64 nothing is rounded: the model is the oracle on ``build_problem``'s own G and detJ, to ``TOL`` (the geometry kinds: the
    factors formed from the vertices ARE those arrays; the affine kind: on an affine box G[c, q] is G[c, 0] w_q / w_0 to rounding)."""
    tol = TOL[np.dtype(np.float64)]
    for kind in model.KINDS:
        geo = _geo(kind, P, SHAPES[P], np.float64)
        if kind != "affine":
            G, detJ = model.factors(geo, np.float64)
            assert np.array_equal(G, geo["G"]) and np.array_equal(detJ, geo["detJ"])
        c = model.model(kind, geo)
        D, G, detJ, dm = geo["D"], geo["G"], geo["detJ"], geo["dofmap"]
        plain = {k: r["y0"].copy() for k, r in c["out"].items()}
        if kind in STIFFNESS:
            oracle_c.stiffness_apply(P, D, c["x"], geo["cc"], plain["y"], G, dm)
        else:
            for k in ("b", "bs"):
                oracle_c.stiffness_apply(P, D, c["u"], c["c3"], plain[k], G, dm)
                oracle_c.stiffness_apply(P, D, c["v"], c["c4"], plain[k], G, dm)
            oracle_c.mass_apply(c["v"] * c["v"], c["c5"], plain["b"], detJ, dm)
            oracle_c.mass_apply(c["u"], c["c2"], plain["m"], detJ, dm)
        for k, r in c["out"].items():
            assert r["e_cpu"] is None and r["cpu32"] is None
            e2, em = rel_l2(plain[k], r["ref"]), rel_max(plain[k], r["ref"])
            assert e2 < tol["l2"] and em < tol["mx"], (kind, k, e2, em)


def test_the_fp32_oracle_is_within_two_units_of_the_model(cases32):
    """e_cpu, on which the fp32 bar of the GPU tests is built, is an fp32 evaluation's error: below 2 x 2^-23 in rel l2 and in rel max
    for every output of every case of the build matrix and of the one-cell and full-batch cases -- so 8 x max(e_cpu, 2^-23) is below
    16 units, 5 x below ``TOL`` (l2) and 50 x (max)."""
    cases = dict(cases32)
    cases.update({(kind, P, shape): model.model(kind, _geo(kind, P, shape, np.float32)) for kind in model.KINDS for P, shape in EDGE_SHAPES})
    worst = {}
    for key, c in cases.items():
        for k, r in c["out"].items():
            e2, em = r["e_cpu"]
            w = worst.setdefault((key[0], k), [0.0, 0.0])
            w[0], w[1] = max(w[0], e2), max(w[1], em)
            assert 0 < e2 < 2 * U and 0 < em < 2 * U, (key, k, e2 / U, em / U)
    for (kind, k), (e2, em) in worst.items():
        print(f"{kind} {k}: e_cpu up to l2 {e2:.3e} max {em:.3e}")
    tol = TOL[np.dtype(np.float32)]
    assert builds.FP32_MARGIN * 2 * U * 5 < tol["l2"] and builds.FP32_MARGIN * 2 * U * 50 < tol["mx"]


@pytest.mark.parametrize("kind", sorted(model.KINDS))
def test_the_fp32_oracle_on_the_colliding_dofmap(kind):
    """37 cells on 50 dofs: a dof sums about 47 cell contributions, which the oracle adds one by one in fp32.  The bound of
    tests/test_nodal_model64.py for the same dofmap: 4 units in rel l2, 8 in rel max."""
    c = model.model(kind, model.colliding(np.float32, affine=kind == "affine"))
    assert c["ncells"] == 37 and c["ndofs"] == 50
    for k, r in c["out"].items():
        e2, em = r["e_cpu"]
        print(f"{kind} {k}: e_cpu l2 {e2:.3e} max {em:.3e}")
        assert 0.25 * U < e2 < 4 * U and 0.25 * U < em < 8 * U, (kind, k, e2 / U, em / U)


@pytest.mark.parametrize("P", sorted(SHAPES))
def test_the_affine_model_is_the_general_model_on_the_affine_box(oracle_c, cases32, P):
    """The sheared box is affine: all six components of G are non-zero, and G[c, 0] w_q / w_0 applied in fp64 is the fp64 apply of the
    whole G array -- in fp64 to ``TOL``; in fp32 to the rounding of G: every G[c, q] is formed in fp32 and rounded on its own, so is
    G[c, 0] and so is w_q / w_0, a few units of 2^-23 between the two arrays entry by entry, which the apply averages: below 8 units
    (the margin of the fp32 bar) in rel l2."""
    for dtype, bound in ((np.float64, TOL[np.dtype(np.float64)]["l2"]), (np.float32, 8 * U)):
        c = cases32["affine", P] if dtype == np.float32 else model.model("affine", model.affine_box(P, SHAPES[P], dtype))
        G = c["G"].astype(np.float64)
        assert (np.abs(G[:, 0, :]).min(axis=0) > 1e-3 * np.abs(G[:, 0, :]).max()).all()  # (1e-2 on the 11 x 1 x 1 box; a rounded zero: 1e-7)
        assert len(np.unique(np.round(np.abs(G[0, 0, :]) / np.abs(G[0, 0, :]).max(), 3))) == 6
        add = np.zeros(c["ndofs"])
        oracle_c.stiffness_apply(P, c["D"].astype(np.float64), c["x"].astype(np.float64), c["cc"].astype(np.float64), add, G, c["dofmap"])
        e = rel_l2(c["out"]["y"]["add"], add)
        print(f"affine P={P} {np.dtype(dtype).name}: rel l2 {e:.3e}")
        assert e < bound, (P, dtype, e)


# ---- the build matrix of the GPU tests against what the library compiles ---------------------------------------------------------------
_NAME = re.compile(r"fus::(stiffness_plan(?:_rows|_affine|_geom)?_kernel|westervelt_cell(?:_geom)?_kernel)<(double|float), (\d+), (\d+), (.*), (true|false), (true|false)>")


def _compiled_keys():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    keys = []
    for name in ru.parse(ru.cached_remarks()):
        m = _NAME.search(name)
        if m:
            args = tuple(a == "true" if a in ("true", "false") else int(a) for a in m.group(5).split(", "))
            keys.append((m.group(1), m.group(2), int(m.group(3)), args, m.group(6) == "true", m.group(7) == "true"))
    return keys


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_the_build_matrix_is_what_the_library_compiles():
    """Every compiled instantiation of the six kernels maps onto the key of its template arguments (kernel, type, P, ALIAS / PADLDS /
    MINW / ring / PREG / MASS, ORDERED, RUNS); the GPU matrix's cases map onto the same keys through ``template_key``.  The two sets
    are equal and neither holds a key twice: an instantiation added to the library without a case fails here, and so does a case
    that no instantiation stands behind."""
    compiled = _compiled_keys()
    tested = [builds.template_key(b) for b in builds.MATRIX]
    assert len(compiled) == len(set(compiled)) and len(tested) == len(set(tested)), "a key occurs twice"
    missing, unknown = sorted(set(compiled) - set(tested)), sorted(set(tested) - set(compiled))
    assert not missing, f"{len(missing)} compiled instantiations have no case in the build matrix, e.g. {missing[:4]}"
    assert not unknown, f"{len(unknown)} cases of the build matrix name no compiled instantiation, e.g. {unknown[:4]}"
    assert len(tested) == 726 and len(builds.MATRIX) == len(set(builds.MATRIX))
    count = lambda d: [sum(1 for t in tested if t[:2] == (k, d)) for k in builds.KERNEL.values()]  # noqa: E731
    assert count("double") == [108, 14, 40, 40, 80, 80] and count("float") == [124, 0, 40, 40, 80, 80]
