"""tools/measure.py, the parts that need no device: the round schedule, the statistics, the three-spreads bar of docs/history.md 3.2
and its printed line, the interleaving driven by a fake timer, the log tee -- and that every tool ported to it parses its arguments
before it imports torch or does any work (``--help`` in a fresh child process on a machine without a GPU)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402

PORTED = ["ab_plan_rows", "ab_xcd_group", "ab_stiffness", "ab_mass_gather", "ab_mass_exclusive", "ab_vector_stream", "ab_westervelt_gathers",
          "time_gradient", "time_sensors", "time_sources", "time_bioheat", "time_field_monitor", "time_vecops", "time_rk4", "time_rk4_graph",
          "sweep"]
# the pinned rounds (us) of the formatter cases, checked by hand
ARM0 = [227.6, 227.9, 227.4, 227.7, 227.5, 227.8, 227.6]
ARM1_FASTER = [221.2, 221.0, 221.4, 221.1, 221.3, 221.2, 221.2]
ARM1_SAME = [227.4, 227.9, 227.0, 227.5, 227.3, 227.6, 227.2]


def test_round_schedule_alternates_only_when_asked():
    arms = {"a": None, "b": None, "c": None}
    plain, alt = measure.round_schedule(arms, 4, False), measure.round_schedule(arms, 4, True)
    assert plain == [["a", "b", "c"]] * 4
    assert alt == [["a", "b", "c"], ["c", "b", "a"], ["a", "b", "c"], ["c", "b", "a"]]
    for rnd in plain + alt:
        assert sorted(rnd) == ["a", "b", "c"]


def test_stats():
    assert measure.stats([3.0, 1.0, 2.0]) == (2.0, 2.0, 1.0, 3.0)
    assert measure.stats([4.0, 1.0, 2.0, 3.0]) == (2.5, 3.0, 1.0, 4.0)  # even count: the mean of the two middle values
    assert measure.stats([7.0]) == (7.0, 0.0, 7.0, 7.0)
    assert measure.stats([5.0, 5.0, 5.0]).spread == 0.0
    s = measure.stats([1.0, 9.0, 4.0])
    assert (s.median, s.spread, s.min, s.max) == (4.0, 8.0, 1.0, 9.0)


def test_verdict_outcomes_and_boundaries():
    base = [10.0, 11.0, 12.0]  # median 11, spread 2: the bar is 6
    for arm_median, word in ((4.0, "FASTER"), (5.0, "not distinguishable"), (11.0, "not distinguishable"), (17.0, "not distinguishable"),
                             (18.0, "SLOWER")):
        v = measure.verdict(base, [arm_median] * 3)
        assert (v.gain, v.bar, v.word) == (11.0 - arm_median, 6.0, word)


def test_verdict_bar_comes_from_the_larger_spread():
    wide, narrow = [10.0, 11.0, 14.0], [8.0, 8.0, 8.5]
    assert measure.verdict(wide, narrow).bar == 12.0  # the base arm's spread 4 sets it
    assert measure.verdict(narrow, wide).bar == 12.0  # the arm's
    assert measure.verdict(wide, narrow).word == "not distinguishable" and measure.verdict(narrow, wide).word == "not distinguishable"


def test_verdict_factor():
    base, arm = [10.0, 11.0, 12.0], [7.0, 7.0, 7.0]  # gain 4, spread 2
    assert measure.verdict(base, arm).word == "not distinguishable"
    assert measure.verdict(base, arm, factor=1).word == "FASTER" and measure.verdict(base, arm, factor=1).bar == 2.0
    assert measure.verdict(base, arm, factor=2).word == "not distinguishable"  # gain == bar
    assert measure.verdict(arm, base, factor=1).word == "SLOWER"


def test_verdict_line_pinned_faster():
    v = measure.verdict(ARM0, ARM1_FASTER)
    assert (round(v.base_median, 9), round(v.gain, 9), round(v.bar, 9), v.word) == (227.6, 6.4, 1.5, "FASTER")
    assert round(measure.stats(ARM1_FASTER).median, 9) == 221.2 and round(measure.stats(ARM1_FASTER).spread, 9) == 0.4
    assert measure.verdict_line("arm 0", ARM0, "arm 1", ARM1_FASTER) == "arm 0 - arm 1 = +6.40 us (+2.81 %), bar 3 x the larger spread = 1.50 us -> FASTER"
    ms = [[t * 1e-3 for t in arm] for arm in (ARM0, ARM1_FASTER)]  # the same rounds held in ms print the same line
    assert measure.verdict_line("arm 0", ms[0], "arm 1", ms[1], to_us=1e3) == measure.verdict_line("arm 0", ARM0, "arm 1", ARM1_FASTER)


def test_verdict_line_pinned_not_distinguishable():
    v = measure.verdict(ARM0, ARM1_SAME)
    assert (round(measure.stats(ARM1_SAME).median, 9), round(v.gain, 9), round(v.bar, 9)) == (227.4, 0.2, 2.7)
    assert measure.verdict_line("arm 0", ARM0, "arm 1", ARM1_SAME) == ("arm 0 - arm 1 = +0.20 us (+0.09 %), bar 3 x the larger spread = 2.70 us "
                                                                       "-> not distinguishable")


def test_verdict_lines_compare_every_arm_with_the_first():
    lines = measure.verdict_lines({"old": ARM0, "new": ARM1_FASTER, "same": ARM1_SAME})
    assert len(lines) == 2
    assert lines[0] == "  old - new = +6.40 us (+2.81 %), bar 3 x the larger spread = 1.50 us -> FASTER  (spreads 0.50 / 0.40 us)"
    assert measure.verdict_lines({"old": ARM0, "new": ARM1_FASTER}, indent="step: ") == ["step: " + lines[0][2:]]
    assert lines[1] == "  old - same = +0.20 us (+0.09 %), bar 3 x the larger spread = 2.70 us -> not distinguishable  (spreads 0.50 / 0.90 us)"


@pytest.mark.parametrize("alternate", [False, True])
def test_interleave_order(alternate):
    events = []

    def arm(name):
        return (lambda: events.append(("select", name))), (lambda: events.append(("call", name)))

    def timer(fn):  # a fake: one call, and a time that says which call of the run it was
        fn()
        return float(len(events))

    arms = {"a": arm("a"), "b": arm("b"), "c": lambda: events.append(("call", "c"))}  # c has no knobs
    times = measure.interleave(arms, 3, timer, warm=2, alternate=alternate)
    warm, timed = events[:8], events[8:]
    assert warm == [("select", "a"), ("call", "a"), ("call", "a"), ("select", "b"), ("call", "b"), ("call", "b"), ("call", "c"), ("call", "c")]
    order = [n for rnd in measure.round_schedule(arms, 3, alternate) for n in rnd]
    expect, stamps = [], {"a": [], "b": [], "c": []}
    for name in order:
        expect += ([("select", name)] if name != "c" else []) + [("call", name)]
        stamps[name].append(float(8 + len(expect)))
    assert timed == expect  # every select directly before its arm's timed call, nothing timed before the last warm-up
    assert times == stamps  # each time under its arm, in round order
    events.clear()
    assert list(measure.interleave(arms, 1, timer)) == ["a", "b", "c"] and events[0] == ("select", "a") and len(events) == 5  # no warm-up phase


def test_log_tees_to_a_file_and_makes_the_directory(tmp_path, capsys):
    path = tmp_path / "new_dir" / "tool.log"
    with measure.Log("some_tool", str(path)) as log:
        log.header("  (extra)", device="a device", library="abc123")
        log("second line")
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("# tools/some_tool.py on a device, ") and out[0].endswith(", library abc123  (extra)") and out[1] == "second line"
    assert path.read_text().splitlines() == out
    with measure.Log("some_tool", str(path)) as log:
        log("third line")
    assert path.read_text().splitlines() == out + ["third line"]  # appended


def test_log_with_an_empty_path_writes_nothing(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with measure.Log("some_tool", "") as log:
        log("only printed")
    assert capsys.readouterr().out == "only printed\n" and os.listdir(tmp_path) == []


@pytest.mark.parametrize("tool", PORTED)
def test_ported_tool_parses_arguments_before_torch_or_any_work(tool, tmp_path):
    (tmp_path / "torch.py").write_text("raise ImportError('torch imported before the arguments were parsed')\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), "--help"], capture_output=True, text=True, timeout=60,
                       env={**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path)] + os.environ.get("PYTHONPATH", "").split(os.pathsep))})
    assert r.returncode == 0, r.stderr
    assert "usage:" in r.stdout
