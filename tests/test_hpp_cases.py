"""What tests/test_fus_gpu_hpp_gpu.py takes for granted about its cases (tests/hpp_cases.py), without a GPU: the container round-trips,
every floating-point input of a ``float`` case is exact in float, every model passes its own check, and -- the condition that makes the
GPU test ABLE to fail on an exchanged pair of same-typed pointers in a forward of include/fus_gpu.hpp -- the model evaluated with any two
members of a group of interchangeable arguments exchanged differs from the expected output by at least 1000 times the bar that output
is held to.  The groups, by functor:

    Gradient, Nodal, WesterveltNodal    pts, wts (dphi has another shape: a model cannot read it in their place)
    WesterveltNodal                     nodal3, nodal4; c3, c4
    PointProbe, FieldAccumulator        pmax, pmin; hre, him (FieldAccumulator also usq, vsq)
    ElementReceive                      hre, him
    PointSource, FacetSourceArray       amplitude, phase, delay
    FacetSourceArray                    c1, c2 (detJ has another shape)
    BioheatStage                        minv, pr, s; T0, Tn, acc
    RelaxStage                          xi0, xin, acc

Also: tests/host/fus_gpu_hpp_check.cpp names every functor class of the header for both types and all ten degrees, and the driver
tests/host/fus_gpu_hpp_run.cpp switches over the same degrees and types."""

import itertools
import os
import re

import numpy as np
import pytest

import hpp_cases as hc
from conftest import ROOT

FACTOR = 1000.0
TYPES = list(hc.DTYPES.items())
_groups = {}


def _degree(P, name):
    if (P, name) not in _groups:
        _groups[P, name] = {g.name: g for g in hc.degree_groups(P, hc.DTYPES[name])}
    return _groups[P, name]


def _free(name):
    if name not in _groups:
        _groups[name] = {g.name: g for g in hc.free_groups(hc.DTYPES[name])}
    return _groups[name]


def _distance(true, other, dtype):
    """How far the array ``other`` lies from the expected output ``true``, in units of the bar ``true`` is held to; for an "abs" check
    over the entries that have a bar (the written ones) where there are any."""
    if true.kind == "abs":
        ref, oth, bound = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (true.ref, other, true.bound))
        live = bound > 0
        if live.any():
            with np.errstate(invalid="ignore"):
                err = np.where(oth[live] == ref[live], 0.0, np.abs(oth[live] - ref[live]))
            return float(np.max(err / bound[live]))
    return hc.ratio(true, other, dtype)


def _assert_swaps(group, dtype, exchange=hc.exchanged):
    true = group.model(group.inputs)
    seen = 0
    for names, outputs in group.swaps:
        for a, b in itertools.combinations(names, 2):
            other = exchange(group, a, b)
            for k in outputs:
                d = max(_distance(true[j], other[j].ref, dtype) for j in ((k,) if isinstance(k, str) else k))
                assert d >= FACTOR, f"{group.name}: {a} <-> {b} moves {k} by {d:.3g} x its bar only"
                seen += 1
    return seen


def test_container_round_trips(tmp_path):
    entries = {"a.f": np.array([1.5, -2.25, np.inf]), "a.i": np.arange(5, dtype=np.int32), "b.l": np.array([2**40, -1], dtype=np.int64),
               "b.empty": np.zeros(0), "a.name_of_thirty-one_character_": np.ones(3)}
    back = hc.decode(hc.encode(entries))
    assert list(back) == list(entries)
    for k, a in entries.items():
        assert back[k].dtype == a.dtype and np.array_equal(back[k], a)
    with pytest.raises(AssertionError):
        hc.encode({"x" * 32: np.zeros(1)})
    g = hc.Group("g", dict(x=np.arange(3, dtype=np.float32), n=np.array([7], dtype=np.int64)), None, [])
    hc.write_case(tmp_path / "c.bin", [g])
    assert {k: v.tolist() for k, v in hc.read_outputs(tmp_path / "c.bin", "g").items()} == {"x": [0.0, 1.0, 2.0], "n": [7]}
    # the twin the C++ example reads is the same container
    with open(os.path.join(ROOT, "tests", "golden", "ops_P4_2x2x2_pert_float64.bin"), "rb") as f:
        assert int(hc.decode(f.read())["P"][0]) == 4


@pytest.mark.parametrize("P", hc.DEGREES)
def test_every_float_input_is_exact_in_float(P):
    for g in list(_degree(P, "float").values()) + (list(_free("float").values()) if P == 4 else []):
        for k, a in g.inputs.items():
            a = np.asarray(a)
            if a.dtype.kind == "f":
                with np.errstate(over="ignore"):
                    assert np.array_equal(a.astype(np.float64), a.astype(np.float64).astype(np.float32).astype(np.float64)), f"{g.name}.{k}"
            else:
                assert a.dtype in (np.int32, np.int64), f"{g.name}.{k}"
            assert len(f"{g.name}.{k}") < 32


@pytest.mark.parametrize("name,dtype", TYPES)
@pytest.mark.parametrize("P", hc.DEGREES)
def test_exchanged_arguments_of_the_degree_functors_are_visible(P, name, dtype):
    groups = _degree(P, name)
    assert set(groups) == {"cell", "coll", "probe", "psrc"} | ({"decl"} if P == 1 else set())
    assert sum(_assert_swaps(g, dtype) for g in groups.values()) == 5 + 1 + 1 + 2 * 2 + 3


@pytest.mark.parametrize("name,dtype", TYPES)
def test_exchanged_arguments_of_the_degree_free_functors_are_visible(name, dtype):
    groups = _free(name)
    assert set(groups) == {"facet", "recv", "mon_a", "mon_s", "bio_a", "bio_s", "rel_a", "rel_s", "loop"}
    for g in groups.values():
        stage = g.name[:3] in ("bio", "rel")
        assert _assert_swaps(g, dtype, hc.stage_exchanged if stage else hc.exchanged) > 0 or g.name == "loop"


@pytest.mark.parametrize("name,dtype", TYPES)
def test_every_model_passes_its_own_check(name, dtype):
    """``verify`` on the expected arrays themselves (what a perfect driver would write): every check, the bitwise and the
    self-referring ones included, accepts them -- and rejects them with one entry moved."""
    for g in list(_degree(2, name).values()) + list(_free(name).values()):
        if g.name == "loop":
            continue  # (its expected result is the CPU loop's, held by tests/test_bioheat_gpu.py's own check)
        exp = g.model(g.inputs)
        got = {k: np.array(c.ref, dtype=np.float64).reshape(-1) for k, c in exp.items() if c.kind in ("tol", "abs", "bits")}
        for k, c in exp.items():
            if c.kind == "same" and not k.endswith("_same"):
                got[k] = got[c.ref]
        if g.name[:3] == "bio":  # the dose and the peak are formed from the stage's own T0
            n = int(g.inputs["nlocal"][0])
            for tag, st, variant in hc.BIOHEAT_RUNS:
                if st == 3 and variant != "bare":
                    T = got[f"{tag}.T0"][:n]
                    init = variant == "init"
                    got[f"{tag}.tmax"] = T if init else np.maximum(np.asarray(g.inputs["tmax"], dtype=np.float64), T)
                    got[f"{tag}.cem43"] = hc.bioheat_cpu.dose_increment(T, float(g.inputs["scalars"][0])) + (0.0 if init else g.inputs["cem43"])
        figures = {}
        hc.verify(g, got, dtype, figures)
        assert figures and max(figures.values()) <= 1.0
        k = next(k for k, c in exp.items() if c.kind in ("tol", "abs") and np.size(c.ref))
        bad = dict(got)
        bad[k] = got[k].copy()
        bad[k][np.argmax(np.abs(got[k]))] *= 1.01
        with pytest.raises(AssertionError):
            hc.verify(g, bad, dtype)


def test_the_stage_models_take_the_tableau_from_the_package():
    from conftest import pkg

    sb = pkg("solver_base")
    assert [hc.tableau(i, 0.5, np.float64) for i in range(4)] == [(sb.B_RUNGE[0] * 0.5, sb.A_RUNGE[1] * 0.5, 0), (sb.B_RUNGE[1] * 0.5, sb.A_RUNGE[2] * 0.5, 1),
                                                                  (sb.B_RUNGE[2] * 0.5, sb.A_RUNGE[3] * 0.5, 1), (sb.B_RUNGE[3] * 0.5, 0.0, 2)]
    assert sb.A_RUNGE == (0.0, 0.5, 0.5, 1.0) and sb.B_RUNGE == (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)  # classical RK4


def test_the_compile_check_names_every_functor_class_type_and_degree():
    header = open(os.path.join(ROOT, "include", "fus_gpu.hpp")).read()
    check = open(os.path.join(ROOT, "tests", "host", "fus_gpu_hpp_check.cpp")).read()
    public = header[header.index("}  // namespace detail"):]
    with_degree = re.findall(r"template <typename T, int P>\s*class (\w+)", public)
    without = re.findall(r"template <typename T>\s*class (\w+)", public)
    assert len(with_degree) == 7 and len(without) == 5
    degrees = [int(d) for d in re.findall(r"template class fus_gpu::X<T, (\d+)>;", check)]
    assert degrees == list(range(1, 11))
    for c in with_degree:
        assert f"FUS_CHECK_DEGREES({c}, T)" in check, c
    for c in without:
        assert f"template class fus_gpu::{c}<T>;" in check, c
    assert "FUS_CHECK_TYPE(double)" in check and "FUS_CHECK_TYPE(float)" in check


def test_the_driver_dispatches_every_degree_and_both_types():
    """(tests/test_fus_gpu_hpp_gpu.py compiles it, with -Wall -Wextra -Werror.)"""
    text = open(os.path.join(ROOT, "tests", "host", "fus_gpu_hpp_run.cpp")).read()
    for P in range(1, 11):
        assert f"case {P}: run_one<T, {P}>" in text
    assert "return run<double>(" in text and "return run<float>(" in text and "__global__" not in text
