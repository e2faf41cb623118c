"""The tools ported to tools/measure.py, run in-process through their ``main([...])`` on one MI355X at the smallest sizes at which their
own code paths all run (a plan with more than one batch, the rows kernel shipping at fp64 P = 2, a gather plan at P = 3), and
``event_time`` itself.  What is checked is the tools' output and what they leave behind, not a time: workload sizes belong to manual
runs."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import TOL, pkg

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
FLOAT = r"[-+]?\d+\.\d+(?:e[-+]?\d+)?"


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(autouse=True)
def _fresh_plans_and_knobs(gpu):
    lib, ops = pkg("_lib"), pkg("operators")
    knobs = {k: lib.get_tuning(k) for k in range(1, 9)}
    ops._PLANS.clear()
    ops.use_plan(True)
    yield
    for k, v in knobs.items():
        lib.set_tuning(k, v)
    ops.use_plan(True)
    ops._PLANS.clear()


def run_tool(name, argv, capsys):
    assert importlib.import_module(name).main(argv) in (None, 0)
    return capsys.readouterr().out.splitlines()


def check_verdict_tool(out, arms, agree):
    assert len([ln for ln in out if re.search(rf"median +{FLOAT} us  spread +{FLOAT} us", ln)]) == arms
    verdicts = [ln for ln in out if re.search(rf"= {FLOAT} us \({FLOAT} %\), bar 3 x the larger spread = {FLOAT} us -> (FASTER|SLOWER|not distinguishable)$", ln)]
    assert len(verdicts) == arms - 1
    (diff,) = [float(m.group(1)) for ln in out if (m := re.search(agree + rf" = ({FLOAT})", ln))]
    assert diff <= TOL[np.dtype(np.float64)]["l2"]  # 1e-12


def test_ab_plan_rows(capsys):
    lib = pkg("_lib")
    out = run_tool("ab_plan_rows", ["--config", "2:6", "--rounds", "7", "--log", ""], capsys)
    check_verdict_tool(out, 2, r"max \|y1 - y0\| / max \|y0\|")
    assert "rows_consecutive 1" in "\n".join(out)  # the rows kernel is what arm 1 ran
    assert lib.get_tuning(lib.TUNE_PLAN_ROWS) == 1


def test_ab_xcd_group(capsys):
    lib = pkg("_lib")
    out = run_tool("ab_xcd_group", ["--config", "2:8", "--groups", "8", "--rounds", "7", "--no-model", "--log", ""], capsys)
    check_verdict_tool(out, 3, r"max \|y - y_g0\| / max \|y_g0\|")
    assert len([ln for ln in out if ln.strip().startswith("rounds ") and len(ln.split()) == 8]) == 3
    assert (lib.get_tuning(lib.TUNE_XCD_REMAP), lib.get_tuning(lib.TUNE_PLAN_XCD_GROUP)) == (0, -1)


def test_ab_stiffness(capsys):
    out = run_tool("ab_stiffness", ["--degree", "2", "--cells", "6", "--rounds", "3", "--reps", "5", "plan", "plan:0", "col:0"], capsys)
    assert len([ln for ln in out if re.match(r"^plan\s*: median \d+\.\d{4} ms  min \d+\.\d{4} ms", ln)]) == 1
    rounds = [ln for ln in out if ln.strip().startswith("rounds:")]
    assert len(rounds) == 3 and all(len(ln.split()) == 1 + 3 for ln in rounds)
    assert len([ln for ln in out if re.search(r"plan - (plan:0|col:0) = .* -> (FASTER|SLOWER|not distinguishable)  \(spreads ", ln)]) == 2


def test_ab_mass_gather(capsys):
    out = run_tool("ab_mass_gather", ["--degree", "3", "--cells", "5", "--rounds", "3", "--reps", "5"], capsys)
    for start in ("plan", "gather:0"):
        assert len([ln for ln in out if re.match(rf"^{start}\s*: median \d+\.\d{{4}} ms  min \d+\.\d{{4}} ms", ln)]) == 1
    equal = [ln for ln in out if "bitwise equal:" in ln]
    assert equal and all(ln.endswith("bitwise equal: True") for ln in equal)
    assert [ln for ln in out if re.search(r"plan - gather:0 = .* -> (FASTER|SLOWER|not distinguishable)  \(spreads ", ln)]


def test_time_gradient(capsys):
    out = run_tool("time_gradient", ["--configs", "2:6", "--rounds", "3", "--log", ""], capsys)
    results = [ln for ln in out if ln.endswith("x the stiffness apply")]
    assert [ln.split()[2:4] for ln in results] == [[t, k] for t in ("float64", "float32") for k in ("stiffness_plan_geom", "gradient_plan_geom")]
    assert all(re.search(rf"us \(min {FLOAT}, max {FLOAT}, spread \d+\.\d{{2}}\)  model", ln) for ln in results)  # what the port added
    assert not [ln for ln in out if "->" in ln or "FASTER" in ln or "SLOWER" in ln or "distinguishable" in ln]  # two kernels, not two arms: no verdict
    assert out[0].startswith("# tools/time_gradient.py on ") and ", library " in out[0]


def test_sweep(capsys):
    out = run_tool("sweep", ["--dofs", "4000", "--degrees", "2", "--dtypes", "f64", "--reps", "5"], capsys)
    (line,) = [ln for ln in out if ln.startswith("P=2 N=7 f64 cells=343 dofs=3375: ")]
    assert [f.split(" ")[0] for f in line.split(": ", 1)[1].split(" | ")] == ["K[plan]", "K[atomic]", "K[in-kernel", "M", "M[static", "M[atomic]"]
    assert all(float(t) > 0 for t in re.findall(rf"({FLOAT}) ms", line))


def test_event_time_of_a_fill(gpu):
    import measure

    buf = gpu.empty(1 << 18, dtype=gpu.float32, device="cuda")  # 1 MiB
    ms = measure.event_time(lambda: buf.fill_(1.0), 20, warm=2)
    assert ms > 0.0
    assert measure.event_time_isolated(lambda: buf.fill_(1.0), 5) > 0.0 and measure.host_time(lambda: buf.fill_(1.0)) > 0.0


@pytest.mark.parametrize("timer", ["event_time", "event_time_isolated"])
def test_event_time_runs_exactly_warm_plus_reps_calls(gpu, timer):
    import measure

    buf, calls = gpu.zeros(16, device="cuda"), []

    def fn():
        calls.append(1)
        buf.add_(1.0)

    getattr(measure, timer)(fn, 7, warm=3)
    assert len(calls) == 10 and float(buf[0]) == 10.0
    calls.clear()
    getattr(measure, timer)(fn, 4)
    assert len(calls) == 4
