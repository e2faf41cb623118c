"""Every functor class of include/fus_gpu.hpp on the device, in float and double and at every degree, against the fp64 models of
tests/hpp_cases.py.  tests/host/fus_gpu_hpp_run.cpp -- a plain C++ user of the header, linked against libfusgpu.so -- is compiled once,
then run as a child process per (P, type): it reads a case file, applies the functors and writes every output array; this module holds
the models and the bars (tests/hpp_cases.py names them per functor; none is wider than the bar of the entry point's own kernel test).
tests/test_hpp_cases.py shows without a GPU that an exchanged pair of same-typed pointers in any forward moves an output by at least
1000 bars.  A child that ends by a signal, an abort or its time limit fails the test; nothing is retried.

Each run prints the driver's log (one line per functor call) and, per output, the error over its bar."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import hpp_cases as hc
from conftest import ROOT

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc")
CASES = [(P, t) for t in hc.DTYPES for P in hc.DEGREES]

# what the log of a run must name (every class, and every member of the table of the issue that added this test)
DEGREE_CALLS = ["StiffnessSpectral3D(Geometry)", "StiffnessSpectral3D(G)", "StiffnessSpectral3D::operator()", "StiffnessSpectral3D::G()",
                "MassSpectral3D(Geometry)", "MassSpectral3D(detJ)", "MassSpectral3D::apply_atomic", "MassSpectral3D::operator() [atomic kernel]",
                "MassSpectral3D::enable_gather(kStaticNever)", "MassSpectral3D::operator() [gather]", "MassSpectral3D::operator() [gather, static detJ]",
                "caller-owned detJ: no snapshot", "MassSpectral3D::enable_gather(kStaticAlways)", "MassSpectral3D::enable_gather() a second time",
                "GradientSpectral3D::operator() [ystride > ndofs]", "NodalStiffnessSpectral3D::operator()", "WesterveltNodalStiffnessSpectral3D::operator()",
                "PointProbe::operator() [short form]", "PointProbe::operator() [capacity 4, slot 2, peaks, H = 2]", "PointSource::operator()"]
FREE_CALLS = ["FacetSourceArray::operator() [c2; set B given, xB null]", "FacetSourceArray::device_stage", "FacetSourceArray::operator() [no c2; set B with xB]",
              "ElementReceive::operator()", "FieldAccumulator::operator() [init", "FieldAccumulator::operator() [H = 2", "[composed RK4 loop]"] + \
             [f"BioheatStage::operator() stage {i}" for i in range(4)] + ["[pr, s, cem43, tmax, init]", "[bare]"] + \
             [f"RelaxStage::operator() stage {i} nr {nr}" for i in range(4) for nr in (1, 4)] + ["[per-dof kappa]", "[kappa null: kappa_scalar]"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/host/fus_gpu_hpp_run.cpp compiled once against the library of this tree."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("hpp_run") / "fus_gpu_hpp_run")
    b = subprocess.run([hipcc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "host", "fus_gpu_hpp_run.cpp"), "-L", CSRC, "-lfusgpu", f"-Wl,-rpath,{CSRC}"],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout + b.stderr
    return exe


def _child(args, limit=120):
    """One run of the driver: a time limit, and any end but exit status 0 fails the test (a negative status is a signal)."""
    try:
        r = subprocess.run(args, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"{' '.join(args[1:])}: no end after {limit} s\n{e.stdout}\n{e.stderr}")
    print(r.stdout)
    assert r.returncode == 0, f"{' '.join(args[1:])}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    return r.stdout


def _run(driver, tmp_path, P, type_name, groups, calls):
    dtype = hc.DTYPES[type_name]
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    hc.write_case(case, groups)
    log = _child([driver, type_name, str(P), case, out])
    lines = [ln for ln in log.splitlines() if ln.startswith(f"[{type_name} P={P}] ")]
    for c in calls:
        assert any(c in ln for ln in lines), f"the log names no call of {c}"
    figures, failures = {}, []
    for g in groups:
        try:
            hc.verify(g, hc.read_outputs(out, g.name), dtype, figures)
        except AssertionError as e:
            failures.append(str(e))
    worst = {}
    for k, v in figures.items():
        worst[k.split(".")[0]] = max(worst.get(k.split(".")[0], 0.0), v)
    print(f"{type_name} P={P}: largest error over its bar per group: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    print("\n".join(f"  {k}: {v:.3g}" for k, v in figures.items()))
    assert not failures, "\n".join(failures)
    return lines


@pytest.mark.parametrize("P,type_name", CASES, ids=[f"P{P}-{t}" for P, t in CASES])
def test_degree_functors_against_the_fp64_models(driver, tmp_path, P, type_name):
    """Mass (every route: atomic, gather, static detJ, caller-owned detJ, a declined gather plan), Stiffness (both constructors, G()),
    Gradient, NodalStiffness, WesterveltNodalStiffness, PointProbe (both forms) and PointSource at degree P."""
    groups = hc.degree_groups(P, hc.DTYPES[type_name])
    lines = _run(driver, tmp_path, P, type_name, groups, DEGREE_CALLS)
    declined = [ln for ln in lines if "gather declined: atomic kernel" in ln]
    coll = next(g for g in groups if g.name == "coll")
    assert bool(declined) == (P == 1 or not coll.model(coll.inputs)["flags"].ref[0])


@pytest.mark.parametrize("type_name", list(hc.DTYPES))
def test_degree_free_functors_against_the_fp64_models(driver, tmp_path, type_name):
    """FacetSourceArray, ElementReceive, FieldAccumulator, BioheatStage and RelaxStage (the three streaming ones 16-byte aligned and
    sliced one element in), and three RK4 steps of StiffnessSpectral3D<T, 4> + BioheatStage against the CPU loop."""
    _run(driver, tmp_path, 4, type_name, hc.free_groups(hc.DTYPES[type_name]), FREE_CALLS)


def test_lifetime_and_refused_constructors(driver, tmp_path):
    """50 rounds of construct / apply / destroy of the five owning functors (Mass with both gather plans) leave the free device memory
    where round 1 left it; each owning constructor, handed a null dofmap, throws std::runtime_error naming fus_plan_build with the
    library's error text -- after its own allocations (the plan workspace; G / detJ) -- and the free memory is back where it was."""
    from conftest import pkg

    case = str(tmp_path / "case.bin")
    hc.write_case(case, [hc.cell_group(4, np.float64)])
    log = _child([driver, "lifetime", "double", "4", case])
    (line,) = [ln for ln in log.splitlines() if ln.startswith("lifetime: free bytes")]
    words = line.replace(":", " ").split()
    first, last = int(words[words.index("1") + 1]), int(words[-1])
    print(f"free bytes after round 1: {first}, after round 50: {last}")
    assert first == last > 0
    text = pkg("_lib").load().fus_error_string(-1).decode()  # FUS_ERR_INVALID_ARGUMENT
    ctors = ["MassSpectral3D(Geometry)", "MassSpectral3D(detJ)", "StiffnessSpectral3D(Geometry)", "StiffnessSpectral3D(G)", "GradientSpectral3D",
             "NodalStiffnessSpectral3D", "WesterveltNodalStiffnessSpectral3D"]
    for c in ctors:
        what, mem = [ln for ln in log.splitlines() if ln.startswith(f"refused {c}: ")]
        assert what == f"refused {c}: fus_plan_build: {text}", what
        w = mem.split()
        assert int(w[w.index("before") + 1]) == int(w[w.index("after") + 1]), mem
