"""The measurement method of this project, written once (the rule's home is docs/history.md 3.2):

    launch each arm ``warm`` times untimed (100 for a kernel A/B), then run rounds of ``reps`` timed launches (200) between ONE event
    pair, the arms alternating in one process; report the median of the round times and their spread (max - min); an arm counts as
    faster only if its median is below the other's by more than THREE times the larger of the two spreads.

Tools put ``tools/`` on ``sys.path`` and ``import measure`` after parsing their arguments; torch is imported inside the functions
that need the device, so the pure parts (``round_schedule``, ``stats``, ``verdict``, ``Log``) run anywhere.

``stats`` takes the statistical median (the mean of the two middle values of an even count).  The tools that used to write
``sorted(v)[len(v) // 2]`` took the upper middle value there; for the odd round counts every tool defaults to the two are the same."""
import collections
import os
import statistics
import time
import types

Stats = collections.namedtuple("Stats", "median spread min max")
Verdict = collections.namedtuple("Verdict", "gain bar base_median word")


def event_time(fn, reps, warm=0):
    """Milliseconds per call of ``fn``: ``warm`` untimed calls, device synchronise, start event, ``reps`` calls, stop event,
    synchronise on the stop event."""
    import torch

    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def event_time_isolated(fn, reps, warm=0):
    """Milliseconds per call with one event pair per launch (launches cannot overlap at their tails): the mean over the pairs."""
    import torch

    for _ in range(warm):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for s, e in evs:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return sum(s.elapsed_time(e) for s, e in evs) / reps


def host_time(fn, per=1):
    """Milliseconds of wall clock around ``fn()`` between two device synchronises, divided by ``per`` (the steps ``fn`` takes)."""
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / per * 1e3


def round_schedule(arms, rounds, alternate=False):
    """The rounds, each the list of arm names in the order they run; with ``alternate`` the odd rounds run in reversed order."""
    names = list(arms)
    return [names[::-1] if alternate and r % 2 else names[:] for r in range(rounds)]


def _arm(entry):
    return entry if isinstance(entry, tuple) else (lambda: None, entry)


def interleave(arms, rounds, timer, warm=None, alternate=False):
    """``{name: [timer(callable) per round]}`` of ``arms`` = {name: callable or (select, callable)}, in one process: first every arm's
    ``warm`` untimed calls (if given), then the rounds of ``round_schedule``.  ``select()`` sets the arm's knobs before its callable
    is warmed and before each of its timed rounds."""
    for select, fn in map(_arm, arms.values() if warm else ()):
        select()
        for _ in range(warm):
            fn()
    times = {name: [] for name in arms}
    for order in round_schedule(arms, rounds, alternate):
        for name in order:
            select, fn = _arm(arms[name])
            select()
            times[name].append(timer(fn))
    return times


def arms_agree(arms, y):
    """One apply per arm into a zeroed ``y``, before anything is timed: the largest max |y - y_first| / max |y_first| over the arms."""
    ys = []
    for select, fn in map(_arm, arms.values()):
        select()
        y.zero_()
        fn()
        ys.append(y.clone())
    return max(float((v - ys[0]).abs().max() / ys[0].abs().max()) for v in ys)


def stats(times):
    """Median (statistical: the mean of the two middle values of an even count), spread (max - min), min and max."""
    return Stats(statistics.median(times), max(times) - min(times), min(times), max(times))


def verdict(base, arm, factor=3):
    """The bar of docs/history.md 3.2 on two arms' round times: gain = median(base) - median(arm), bar = ``factor`` x the larger
    of the two spreads; FASTER if gain > bar, SLOWER if -gain > bar, else not distinguishable."""
    b, a = stats(base), stats(arm)
    gain, bar = b.median - a.median, factor * max(b.spread, a.spread)
    return Verdict(gain, bar, b.median, "FASTER" if gain > bar else "SLOWER" if -gain > bar else "not distinguishable")


def verdict_line(base_name, base, name, arm, to_us=1.0, factor=3):
    """The verdict as the tools print it: gain in us and %, the bar, the word (``to_us``: what turns the times into us)."""
    v = verdict(base, arm, factor)
    return (f"{base_name} - {name} = {v.gain * to_us:+.2f} us ({100 * v.gain / v.base_median:+.2f} %), "
            f"bar {factor} x the larger spread = {v.bar * to_us:.2f} us -> {v.word}")


def verdict_lines(times, to_us=1.0, factor=3, indent="  "):
    """For a tool that compares arms: every arm after the first against the first, with the spreads the bar is made of."""
    (first, base), *rest = times.items()
    return [f"{indent}{verdict_line(first, base, name, v, to_us, factor)}  (spreads {stats(base).spread * to_us:.2f} / {stats(v).spread * to_us:.2f} us)"
            for name, v in rest]


def library_hash():
    """The source hash the loaded libfusgpu.so was built from, ``?`` for a library without one."""
    import fusgpu_loader

    clib = fusgpu_loader.submodule("_lib").load()
    return clib.fus_source_hash().decode() if hasattr(clib, "fus_source_hash") else "?"


class Log:
    """A tee: ``log(s)`` prints and remembers; leaving the context appends what it remembers to ``path`` (``''``: no file)."""

    def __init__(self, tool, path):
        self.tool, self.path, self.lines = tool, path, []

    def __call__(self, s):
        print(s, flush=True)
        self.lines.append(s)

    def header(self, extra="", device=None, library=None):
        if device is None:
            import torch

            device = torch.cuda.get_device_name(0)
        self(f"# tools/{self.tool}.py on {device}, {time.strftime('%Y-%m-%d %H:%M:%S')}, library {library or library_hash()}{extra}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.path and self.lines:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            with open(self.path, "a") as f:
                f.write("\n".join(self.lines) + "\n")


def device_problem(P, N, dtype, perturb=0.16, seed=0, G=False, detJ=False):
    """The operator tools' problem on device 0 (config 3: P = 4, N = 54): the perturbed box mesh with ``dm``, ``xd``, ``xg``, the GLL
    tables (fp64), ``G`` / ``detJ`` through the device precompute when asked (formed in fp64, cast to ``dtype``), ``x`` uniform in
    [0, 1), ``cc`` in [0.5, 1.5) and a zeroed ``y``."""
    import numpy as np
    import torch

    import fusgpu_loader

    boxmesh, gll, lib, pre = (fusgpu_loader.submodule(m) for m in ("boxmesh", "gll", "_lib", "precompute"))
    dev, tdt, n = torch.device("cuda", 0), lib.torch_dtype(dtype), P + 1
    mesh = boxmesh.BoxMesh(P, N, perturb=perturb, seed=seed)
    pts, wts, D = gll.tabulate_1d(P, np.float64)
    dm, xd, xg = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (mesh.dofmap, mesh.x_dofs, mesh.x_g))
    p = types.SimpleNamespace(P=P, N=N, n=n, mesh=mesh, pts=pts, wts=wts, D=D, dev=dev, tdt=tdt, dm=dm, xd=xd, xg=xg, G=None, detJ=None)
    tables = (torch.from_numpy(pre.tabulate_hex_p1_gradients(gll.tensor_points_3d(pts))).to(dev), torch.from_numpy(gll.tensor_weights_3d(wts)).to(dev))
    if G:
        p.G = torch.empty((mesh.ncells, n**3, 6), dtype=torch.float64, device=dev)
        pre.compute_scaled_geometrical_factor_device(p.G, (xd, xg), mesh.ncells, *tables)
        p.G = p.G.to(tdt)
    if detJ:
        p.detJ = torch.empty((mesh.ncells, n**3), dtype=torch.float64, device=dev)
        pre.compute_scaled_jacobian_determinant_device(p.detJ, (xd, xg), mesh.ncells, *tables)
        p.detJ = p.detJ.to(tdt)
    p.x = torch.rand(mesh.ndofs, dtype=tdt, device=dev)
    p.cc = 0.5 + torch.rand(mesh.ncells, dtype=tdt, device=dev)
    p.y = torch.zeros(mesh.ndofs, dtype=tdt, device=dev)
    return p
