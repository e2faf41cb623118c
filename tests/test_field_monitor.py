"""Full-field monitors (field_monitor.FieldMonitor, csrc/field_monitor.hpp), the parts that need no GPU: argument errors, the
plan of recorded steps, merging per-rank focus records, and the register allocation of every kernel instantiation."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg


def test_constructor_errors():
    fm = pkg("field_monitor")
    with pytest.raises(ValueError, match="frequency"):
        fm.FieldMonitor(10, np.float64, harmonics=(1, 2))
    with pytest.raises(ValueError, match="at most 4"):
        fm.FieldMonitor(10, np.float64, harmonics=(1, 2, 3, 4, 5), frequency=1e6)
    with pytest.raises(ValueError, match="at most 4"):
        fm.FieldMonitor(10, np.float64, harmonics=(k for k in range(1, 6)), frequency=1e6)  # any iterable, as before
    with pytest.raises(ValueError, match="mean_square"):
        fm.FieldMonitor(10, np.float64, mean_square=("u", "w"))
    with pytest.raises(ValueError):
        fm.FieldMonitor(-1, np.float64)
    with pytest.raises(TypeError):
        fm.FieldMonitor(10, np.float16, peak=True)


def _sensor_plan(start_time, final_time, dt, max_steps, record_from, capacity=0, nrec=0):
    """The steps PointSensors.expect_steps selects (sensors.py) for a series of ``capacity`` rows of which ``nrec`` are written
    (no series: room for 1 << 16), the rule written out."""
    rk4_steps = pkg("solver_base").rk4_steps
    rf = -np.inf if record_from is None else float(record_from)
    room = capacity - nrec if capacity else 1 << 16
    ends = []
    for t, h in rk4_steps(start_time, final_time, dt, max_steps):
        if len(ends) >= room:
            break
        if t + h > rf:
            ends.append(t + h)
    return ends


@pytest.mark.parametrize("case", [
    (0.0, 1.0e-5, 1.3e-7, None, None),
    (0.0, 1.0e-5, 1.3e-7, 20, 9.05e-7),
    (2.0e-6, 1.0e-5, 1.3e-7, None, 9.0e-6),     # a shortened last step
    (0.0, 1.0e-6, 1.0e-7, None, 5.0e-7),        # record_from on (or next to) a step end
    (0.0, 1.0e-6, 1.0e-7, 3, 5.0e-7),           # nothing to record
    (0.0, 0.0, 1.0e-7, None, None),
])
def test_record_times_are_the_steps_the_time_loop_records(case):
    fm = pkg("field_monitor")
    t0, tf, dt, ms, rf = case
    got = fm.record_times(t0, tf, dt, ms, rf)
    assert got == _sensor_plan(t0, tf, dt, ms, rf)  # bitwise: record() matches its time against these
    # and they are the sums the loop of rk4_schedule forms
    t, n, ends = float(t0), 0, []
    while t < tf and (ms is None or n < ms):
        h = min(dt, tf - t)
        t, n = t + h, n + 1
        if rf is None or t > rf:
            ends.append(t)
    assert got == ends
    if got and ms is None:
        assert got[-1] == tf or abs(got[-1] - tf) <= 1e-15 * tf
    for k in (0, 1, 3, 10**6):  # limit: the first k of them
        assert fm.record_times(t0, tf, dt, ms, rf, limit=k) == got[:k]
    for capacity, nrec in ((5, 0), (5, 2), (5, 5), (len(got) + 1, 1), (0, 0)):  # the room a PointSensors series has left
        room = capacity - nrec if capacity else 1 << 16
        assert fm.record_times(t0, tf, dt, ms, rf, limit=room) == _sensor_plan(t0, tf, dt, ms, rf, capacity, nrec)


def test_merge_focus_of_hand_made_records():
    fm = pkg("field_monitor")
    r0 = {"max": 4.0, "dof": 7, "rank": 0, "position": (0.1, 0.2, 0.3), "level": 0.5, "volume": 3.0,
          "values": np.array([4.0, 2.5, 2.0]), "volumes": np.array([1.0, 1.0, 1.0])}
    r1 = {"max": 10.0, "dof": 3, "rank": 1, "position": (0.4, 0.5, 0.6), "level": 0.5, "volume": 0.75,
          "values": np.array([10.0, 6.0, 5.0]), "volumes": np.array([0.25, 0.25, 0.25])}
    r2 = {"max": 10.0, "dof": 11, "rank": 2, "position": (0.7, 0.8, 0.9), "level": 0.5, "volume": 0.5,
          "values": np.array([10.0]), "volumes": np.array([0.5])}
    r3 = {"max": -np.inf, "dof": -1, "rank": 3, "position": None, "level": 0.5, "volume": 0.0, "values": np.zeros(0), "volumes": np.zeros(0)}
    m = fm.merge_focus([r0, r1, r2, r3])
    assert (m["max"], m["dof"], m["rank"], m["position"]) == (10.0, 3, 1, (0.4, 0.5, 0.6))  # the lowest rank among equal maxima
    assert m["volume"] == 0.75 + 0.5  # threshold 5.0: nothing of rank 0, all of ranks 1 and 2 (5.0 itself counts)
    assert m["level"] == 0.5 and m["values"] is None
    assert fm.FieldMonitor.merge_focus([r0])["volume"] == 3.0 and fm.merge_focus([r3, r0])["rank"] == 0
    assert fm.merge_focus([r2, r1])["rank"] == 1  # order of the list does not matter
    with pytest.raises(ValueError):
        fm.merge_focus([])
    with pytest.raises(ValueError):
        fm.merge_focus([r0, dict(r1, level=0.25)])
    with pytest.raises(ValueError):
        fm.merge_focus([m])  # a reduced record has no candidates left


def test_signature_and_header_agree():
    lib = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "fus_gpu.h")).read()
    for suf in ("f64", "f32"):
        name = f"fus_field_accumulate_{suf}"
        decl = re.search(rf"int {name}\(([^;]*)\);", hdr).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[name]) == 14


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_every_instantiation_keeps_eight_waves_and_no_scratch():
    """Streaming kernels hide HBM latency with resident waves: every field_accumulate_kernel<T, H, W, NT> fits 64 VGPRs (8 waves
    per SIMD on gfx950) and spills nothing -- H = 4 with every output on holds 56 registers of accumulators."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    table = ru.parse(ru.cached_remarks())
    hits = {k: v for k, v in table.items() if "field_accumulate_kernel<" in k}
    seen = set()
    for k, d in hits.items():
        T, H, W, NT = re.search(r"field_accumulate_kernel<(\w+), (\d), (\d), (\d)>", k).groups()
        seen.add((T, int(H), int(W), int(NT)))
        assert d["scratch"] == 0 and d["lds"] == 0 and d["agpr"] == 0, (k, d)
        assert d["occupancy"] >= 8 and d["vgpr"] <= 64, (k, d)
    want = {(T, H, W, NT) for T, Wv in (("double", 2), ("float", 4)) for H in range(5) for W in (1, Wv) for NT in range(3)}
    assert seen == want
    assert hits[next(k for k in hits if "<double, 4, 2, 1>" in k)]["vgpr"] < 64
