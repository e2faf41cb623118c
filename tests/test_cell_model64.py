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


# ---- the mass, column and gradient kernels (tests/cell_op_builds.py, tests/test_cell_op_builds_gpu.py) ----------------------------------
import importlib  # noqa: E402

import cell_op_builds as ob  # noqa: E402

_OP_NAME = re.compile(r"fus::(gradient_plan_geom_kernel|stiffness_col_kernel|mass_plan_kernel|mass_kernel|probe_eval_kernel|point_source_kernel|"
                      r"point_source_wave_kernel)<(double|float), ([^>]*)>\(")


def _compiled_op_keys():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    word = lambda a: a == "true" if a in ("true", "false") else int(a) if a.lstrip("-").isdigit() else a  # noqa: E731
    keys = []
    for name in ru.parse(ru.cached_remarks()):
        m = _OP_NAME.search(name)
        if m:
            keys.append((m.group(1), m.group(2), tuple(word(a) for a in m.group(3).split(", "))))
    return keys


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_the_cell_operator_matrix_is_what_the_library_compiles():
    """The 160 cases of tests/cell_op_builds.py against the compiled instantiations of the four kernels, both ways and each once:
    80 / 40 / 36 / 4.  And the degree list of each point kernel's own GPU test against that kernel's 20 compiled (T, P) pairs (no
    point kernel refuses P = 1 in Python: all three lists are 1 .. 10)."""
    compiled = _compiled_op_keys()
    assert len(compiled) == len(set(compiled))
    cells = [k for k in compiled if k[0] in ob.COUNTS]
    tested = [ob.template_key(b) for b in ob.MATRIX]
    assert len(tested) == len(set(tested)) and len(ob.MATRIX) == len(set(ob.MATRIX)), "a key occurs twice"
    missing, unknown = sorted(set(cells) - set(tested), key=str), sorted(set(tested) - set(cells), key=str)
    assert not missing, f"{len(missing)} compiled instantiations have no case in the build matrix, e.g. {missing[:4]}"
    assert not unknown, f"{len(unknown)} cases of the build matrix name no compiled instantiation, e.g. {unknown[:4]}"
    assert {k: sum(1 for t in tested if t[0] == k) for k in ob.COUNTS} == ob.COUNTS and len(tested) == 160
    assert len({ob.case_id(b) for b in ob.MATRIX}) == 160
    for kernel, (module, constant) in ob.POINT_KERNELS.items():
        degrees = getattr(importlib.import_module(module), constant)
        pairs = sorted((t, P) for t in ("double", "float") for P in degrees)
        assert len(degrees) == len(set(degrees)) and pairs == sorted((k[1], k[2][0]) for k in compiled if k[0] == kernel), kernel
        assert len(pairs) == 20


def test_the_shapes_of_the_cell_operator_matrix_keep_their_promises():
    """Column kernel: at least 9 workgroups, never a multiple of 8, a partial last workgroup where CPB > 1, the block counts cover every
    residue 1 .. 7 mod 8, a live ``lc < CPB`` guard at most degrees, and ``remap_block`` is a bijection at every block count used.
    Planned mass: both shapes of a bucket fall into it, the first at the bucket's lowest ept and the second at its largest N x epb, the
    two ends (M = 256 and M = 4096 exactly) are there, at least three batches with a ragged last one, and 64 KiB of dynamic LDS at
    M = 4096 in fp64.  The Python route: every box holds the 2^15 entries of the planned route, with the EPT the issue's table names.
    mass_kernel: one trip more than the grid holds, and 2^31 entries."""
    residues, guarded = set(), 0
    for (P, target), shape in ob.COL_SHAPES.items():
        cpb, nc = ob.default_cells_per_block(P, target), int(np.prod(shape))
        nb = -(-nc // cpb)
        assert nb >= 9 and nb % 8 != 0 and (cpb == 1 or nc % cpb != 0), (P, target, nb)
        assert sorted(ob.remap_block(b, nb) for b in range(nb)) == list(range(nb))
        residues.add(nb % 8)
        guarded += ob.col_block_threads(P, cpb) > cpb * (P + 1) ** 2
    assert sorted(ob.COL_SHAPES) == sorted((P, t) for P in ob.DEGREES for t in (256, 128))
    assert residues == set(range(1, 8)) and guarded >= 14
    for nb in range(1, 70):
        assert sorted(ob.remap_block(b, nb) for b in range(nb)) == list(range(nb))
    lowest = dict(zip(ob.EPT_LADDER, (1, 2, 3, 4, 5, 6, 7, 9, 12)))
    for bucket, (low, high) in ob.MASS_PLAN_SHAPES.items():
        for s in (low, high):
            N, nent = ob.mass_shape_N(s), ob.mass_shape_entities(s)
            assert N >= 2 and N * s.epb <= ob.PLAN_MAX_ENTRIES and ob.mass_plan_ept(N, s.epb)[1] == bucket
            assert nent > 2 * s.epb and nent % s.epb != 0, (bucket, s)
        assert ob.mass_plan_ept(ob.mass_shape_N(low), low.epb)[0] == lowest[bucket] and ob.mass_shape_N(high) * high.epb == 256 * bucket
    assert sorted(ob.MASS_PLAN_SHAPES) == list(ob.EPT_LADDER)
    assert 4096 * (8 + 8) == 64 << 10  # PlanAcc (a double) and x per entry
    for P in ob.DEGREES:
        N, nc, cpb = (P + 1) ** 3, int(np.prod(ob.MASS_CELL_BOXES[P])), ob.cells_per_batch(P)
        assert N * nc >= ob.MASS_MIN_ENTRIES and nc % cpb != 0 and ob.mass_plan_ept(N, cpb)[1] == ob.MASS_CELL_EPT[P]
        k = ob.mass_facet_box(P)[0]
        Nf = (P + 1) ** 2
        assert (2 * k * k + 4 * k) * Nf >= ob.MASS_MIN_ENTRIES and ob.mass_plan_ept(Nf, ob.entities_per_batch(Nf))[1] == (4 if Nf == 64 else 5)
    assert {e for e in ob.MASS_CELL_EPT.values()} | {4, 5} == {2, 3, 4, 5, 6, 8, 11}  # what Python reaches: neither 1 nor 16
    st, big = ob.MASS_SECOND_TRIP, ob.MASS_BIG
    assert 0 < st["N"] * st["nent"] - ob.MASS_GRID_ENTRIES < 256 * 64 and big["N"] * big["nent"] == 2**31
    assert ob.mass_index_type(big["N"] * big["nent"] // 2) == "unsigned int" and ob.mass_index_type(2**31 - 1) == "long"


OP_EDGE_SHAPES = [(1, (1, 1, 1)), (4, (1, 1, 1)), (10, (1, 1, 1)), (4, (5, 2, 2)), (7, (3, 2, 2))]


@pytest.fixture(scope="module")
def op_cases32():
    """The fp32 model of the two cell kinds at every degree on the shapes of the build matrix and of the edge cases, the facet kind at
    every degree on a 3 x 2 x 2 box, built once."""
    out = {(kind, P, SHAPES[P]): model.model(kind, model.box(P, SHAPES[P], np.float32)) for kind in ("mass", "gradient") for P in sorted(SHAPES)}
    out.update({(kind, P, shape): model.model(kind, model.box(P, shape, np.float32)) for kind in ("mass", "gradient") for P, shape in OP_EDGE_SHAPES})
    out.update({("facet_mass", P, (3, 2, 2)): model.model("facet_mass", model.facet_box(P, (3, 2, 2), np.float32)) for P in sorted(SHAPES)})
    return out


def test_the_new_kinds_keep_the_house_rules(op_cases32):
    """The ids go on from the existing kinds'; x is standard normal and not the smooth field; y0 is a tenth of what is added, per
    output; the arrays are frozen; the facet kind has N = n^2 and touches boundary dofs only."""
    assert sorted(model.OP_KINDS.values()) == [8, 9, 10] and max(model.KINDS.values()) == 7 and not set(model.OP_KINDS) & set(model.KINDS)
    for key, c in op_cases32.items():
        assert c["x"].dtype == np.float32 and c["x"].shape == (c["ndofs"],)
        assert c["ndofs"] < 100 or (0.8 < np.std(c["x"]) < 1.2 and abs(np.mean(c["x"])) < 0.3), key  # (8 draws say little)
        assert set(c["out"]) == (set(model.COMPONENTS) if key[0] == "gradient" else {"y"})
        for k, r in c["out"].items():
            ratio = np.sqrt(np.mean(r["y0"].astype(np.float64) ** 2) / np.mean(r["add"] ** 2))
            assert 0.08 < ratio < 0.12 or c["ndofs"] < 100, (key, k, ratio)
            assert r["ref"].dtype == np.float64 and r["y0"].dtype == r["cpu32"].dtype == np.float32 and not r["ref"].flags.writeable
    c = op_cases32["facet_mass", 3, (3, 2, 2)]
    assert c["dofmap"].shape == (2 * (6 + 4 + 6), 16) and c["detJ"].shape == c["dofmap"].shape and c["detJ"].min() > 0
    assert np.count_nonzero(c["out"]["y"]["add"]) == np.unique(c["dofmap"]).size < c["ndofs"]


@pytest.mark.parametrize("P", [1, 3, 4, 7, 10])
def test_the_fp64_models_of_the_new_kinds_are_the_plain_references(oracle_c, P):
    """In fp64 nothing is rounded: mass is the oracle on ``build_problem``'s detJ, the gradient is ``gradient_cpu.weak_gradient`` on the
    mesh as it stands, both to ``TOL``."""
    import gradient_cpu

    tol = TOL[np.dtype(np.float64)]
    geo = model.box(P, SHAPES[P], np.float64)
    c = model.model("mass", geo)
    plain = c["out"]["y"]["y0"].copy()
    oracle_c.mass_apply(c["x"], geo["cc"], plain, geo["detJ"], geo["dofmap"])
    assert c["out"]["y"]["e_cpu"] is None and rel_l2(plain, c["out"]["y"]["ref"]) < tol["l2"] and rel_max(plain, c["out"]["y"]["ref"]) < tol["mx"]
    g = model.model("gradient", geo)
    y3 = np.stack([g["out"][k]["y0"] for k in model.COMPONENTS]).copy()
    gradient_cpu.weak_gradient(geo["x_dofs"], geo["x_g"], geo["pts"], geo["wts"], geo["D"], geo["dofmap"], g["x"], geo["cc"], geo["ndofs"], y3=y3)
    for d, k in enumerate(model.COMPONENTS):
        assert g["out"][k]["e_bar"] is None and rel_l2(y3[d], g["out"][k]["ref"]) < tol["l2"] and rel_max(y3[d], g["out"][k]["ref"]) < tol["mx"]
    # the three components differ by O(1): a swap of two is an error of order one
    adds = [g["out"][k]["add"] for k in model.COMPONENTS]
    assert min(rel_l2(adds[i], adds[j]) for i in range(3) for j in range(3) if i != j) > 0.5


def test_the_fp32_references_of_the_new_kinds(op_cases32):
    """mass and facet_mass: the fp32 oracle is within two units of 2^-23 of the model, as the other kinds' (``e_bar`` is e_cpu).
    gradient: the fp32 restatement's einsum order is not the kernel's; its error is asserted as it is -- up to P = 5 below 2 units in
    rel l2 and 3 in rel max, on the thin boxes of P >= 6 below 3.5 and 8 (measured: 3.03 and 5.12 at P = 6, 7), never below a tenth of
    a unit -- and ``e_bar``, which enters the bar, is e_cpu capped at 2 units: the fp32 bar of every kind stays at or below 16 units, 5 x below ``TOL`` (l2) and 50 x (max)."""
    worst = {}
    for key, c in op_cases32.items():
        for k, r in c["out"].items():
            e2, em = r["e_cpu"]
            if key[0] == "gradient":
                w = worst.setdefault(key[1], [0.0, 0.0])
                w[0], w[1] = max(w[0], e2), max(w[1], em)
                b2, bm = (2, 3) if key[1] <= 5 or key[2] != SHAPES[key[1]] else (3.5, 8)
                assert 0.1 * U < e2 < b2 * U and 0.1 * U < em < bm * U, (key, k, e2 / U, em / U)
                assert r["e_bar"] == (min(e2, 2 * U), min(em, 2 * U))
            else:
                assert 0 < e2 < 2 * U and 0 < em < 2 * U and r["e_bar"] == r["e_cpu"], (key, k, e2 / U, em / U)
            assert builds.FP32_MARGIN * max(max(r["e_bar"]), U) <= 16 * U
    for P, (e2, em) in sorted(worst.items()):
        print(f"gradient P={P}: e_cpu up to l2 {e2 / U:.2f} max {em / U:.2f} units of 2^-23")
    tol = TOL[np.dtype(np.float32)]
    assert 16 * U * 5 < tol["l2"] and 16 * U * 50 < tol["mx"] and model.E_CAP == 2 * U


@pytest.mark.parametrize("kind", ["mass", "gradient"])
def test_the_fp32_references_of_the_new_kinds_on_the_colliding_dofmap(kind):
    """37 cells on 50 dofs: the bounds of the other kinds on this dofmap, 4 units in rel l2 and 8 in rel max (mass: a dof sums about 47
    products, each rounded once)."""
    c = model.model(kind, model.colliding(np.float32))
    assert c["ncells"] == 37 and c["ndofs"] == 50
    for k, r in c["out"].items():
        e2, em = r["e_cpu"]
        print(f"{kind} {k}: e_cpu l2 {e2 / U:.2f} max {em / U:.2f} units")
        assert 0.1 * U < e2 < 4 * U and 0.1 * U < em < 8 * U, (kind, k, e2 / U, em / U)
