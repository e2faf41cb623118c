#!/usr/bin/env python3
"""What is a line of ``G`` that the memory-side cache still holds worth to the general-G planned stiffness apply?  One operator, one plan,
one x and y at P = 4, 30^3 cells (fp64: G = 162 MB, the whole launch is below the 256 MiB of the cache), two arms alternating in one
process (tools/measure.py):

    arm evicted    the launches rotate over 6 distinct copies of G (972 MB in all): a copy is gone from the cache when its turn comes again
    arm resident   the same G array in every launch

    python tools/probe_g_residency.py [--config 4:30] [--copies 6] [--rounds 9] [--log profiles/probe_g_residency.log]

Same launch shape, plan, x and y in both arms; the sweep direction is pinned upwards (knob ``FUS_TUNE_PLAN_SWEEP`` = 0 where the library has
it).  The ratio t_resident / t_evicted prices a resident line: 1 - ratio, times the share of a config-3 launch that a downward launch can
find resident (tools/model_g_residency.py), is the gain to expect from alternating the sweep direction."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="4:30", help="P:cells-per-direction")
    ap.add_argument("--copies", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=198, help="timed launches per round (a multiple of --copies)")
    ap.add_argument("--no-model", action="store_true", help="skip the CPU model's share of config 3")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "probe_g_residency.log"))
    a = ap.parse_args(argv)
    if a.rounds < 7:
        ap.error("at least 7 rounds")
    if a.reps % a.copies:
        ap.error("--reps must be a multiple of --copies")
    import torch

    import fusgpu_loader
    import measure

    torch.cuda.set_device(0)
    ops, lib = fusgpu_loader.submodule("operators"), fusgpu_loader.submodule("_lib")
    knob = getattr(lib, "TUNE_PLAN_SWEEP", None)
    with measure.Log("probe_g_residency", a.log) as log:
        log.header()
        P, N = (int(v) for v in a.config.split(":"))
        pb = measure.device_problem(P, N, np.float64, G=True)
        mesh = pb.mesh
        op = ops.stiffness_operator(P, pb.D.astype(np.float64).flatten(), np.float64)
        copies = [pb.G] + [pb.G.clone() for _ in range(a.copies - 1)]
        g_mb = pb.G.numel() * 8 / 1e6
        turn = [0]

        def evicted():
            op(pb.x, pb.cc, pb.y, copies[turn[0] % a.copies], pb.dm)
            turn[0] += 1

        def resident():
            op(pb.x, pb.cc, pb.y, pb.G, pb.dm)

        if knob is not None:
            lib.set_tuning(knob, 0)
        arms = {"evicted": evicted, "resident": resident}
        diff = measure.arms_agree(arms, pb.y)
        log(f"P={P} {N}^3 f64: {mesh.ncells} cells, {mesh.ndofs} dofs, G = {g_mb:.1f} MB, {a.copies} copies = {a.copies * g_mb:.1f} MB; "
            f"max |y_resident - y_evicted| / max |y| = {diff:.2e}")
        res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, a.reps) * 1e3, warm=102, alternate=True)  # us
        if knob is not None:
            lib.set_tuning(knob, -1)
        st = {arm: measure.stats(v) for arm, v in res.items()}
        for arm, v in res.items():
            log(f"  arm {arm:>8}: median {st[arm].median:8.2f} us  spread {st[arm].spread:5.2f} us   rounds " + " ".join(f"{t:.2f}" for t in v))
        for line in measure.verdict_lines(res):
            log(line)
        ratio = st["resident"].median / st["evicted"].median
        log(f"  t_resident / t_evicted = {ratio:.4f}: a launch whose G is all resident saves {100 * (1 - ratio):.2f} % "
            f"({st['evicted'].median - st['resident'].median:.2f} us of {g_mb:.0f} MB: {g_mb * 1e6 / max(st['evicted'].median - st['resident'].median, 1e-9) / 1e6:.2f} TB/s of resident G)")
        if not a.no_model:
            import model_g_residency

            r = model_g_residency.model(4, 54)
            share = r["up_down"] / r["g_bytes"]
            # the probe's saving is that of a launch whose G is ALL resident; a config-3 launch has ``share`` of its G resident
            log(f"  config 3 (model, LRU): {r['up_down'] / 1e6:.1f} MB = {100 * share:.1f} % of G resident for a downward launch -> expected gain "
                f"{100 * (1 - ratio) * share:.2f} % of the launch (paper bound: the resident share of the launch's bytes, "
                f"{100 * r['up_down'] / r['launch_bytes']:.1f} %)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
