#!/usr/bin/env python3
"""A/B in one process of the two general-G planned stiffness kernels on one MI355X, at config 3 (fp64, P = 4, 54^3 perturbed cells):

    arm 0   ``FUS_TUNE_PLAN_ROWS`` = 0: stiffness_plan_kernel       (one 16-bit slot per dof, run tables at their full stride)
    arm 1   ``FUS_TUNE_PLAN_ROWS`` = 1: stiffness_plan_rows_kernel  (one 16-bit slot per local row, compact run tables)

    python tools/ab_plan_rows.py [--config 4:54] [--rounds 9] [--log profiles/ab_plan_rows.log]

Same operator object, same plan workspace, same x / G / y; the knob is the only thing that changes between the arms.  Times: HIP events
around back-to-back launches (the method of tools/time_gradient.py): 100 untimed launches of each arm, then rounds of 200 timed launches,
the arms alternating (the order within a round alternates as well).  Reported per arm: the median of the round times and their
spread (max - min).  The bar (docs/history.md): the new arm counts as faster only if its median is below the other
arm's by more than THREE times the larger of the two spreads.

On a tree without the knob (the parent commit) both arms run stiffness_plan_kernel: the run then shows what two arms of the same kernel
differ by.  Index bytes per cell (stated from the layouts, csrc/plan.hpp): arm 0  2 n^3 + 1024 / CPB,  arm 1  2 n^2 + 8 run_stride / CPB."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="4:54", help="P:cells-per-direction")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ab_plan_rows.log"))
    a = ap.parse_args(argv)
    if a.rounds < 7:
        ap.error("at least 7 rounds")
    import torch

    import fusgpu_loader
    import measure

    torch.cuda.set_device(0)
    ops, lib = fusgpu_loader.submodule("operators"), fusgpu_loader.submodule("_lib")
    knob = getattr(lib, "TUNE_PLAN_ROWS", None)
    with measure.Log("ab_plan_rows", a.log) as log:
        log.header("" if knob is not None else "  (no TUNE_PLAN_ROWS in this tree: both arms run stiffness_plan_kernel)")
        P, N = (int(v) for v in a.config.split(":"))
        n = P + 1
        pb = measure.device_problem(P, N, np.float64, G=True)
        mesh = pb.mesh
        op = ops.stiffness_operator(P, pb.D.flatten(), np.float64)

        def set_arm(v):
            if knob is not None:
                lib.set_tuning(knob, v)

        def one():
            op(pb.x, pb.cc, pb.y, pb.G, pb.dm)

        arms = {f"arm {v}": (lambda v=v: set_arm(v), one) for v in (0, 1)}
        diff = measure.arms_agree(arms, pb.y)
        (ws, _, epb), = [v for k, v in ops._PLANS._plans.items() if k[-1] != "strips"]
        hdr = ws[:256].cpu().numpy().view(np.int64)
        rows, stride = int(hdr[8]), int(hdr[9])
        log(f"P={P} {N}^3 fp64: {mesh.ncells} cells, {mesh.ndofs} dofs, plan {ws.numel() / 1e6:.1f} MB, rows_consecutive {rows}, run_stride {stride}, "
            f"max |y1 - y0| / max |y0| = {diff:.2e}")
        idx0 = 2 * n**3 + 1024 / epb
        idx1 = 2 * n**2 + 8 * stride / epb if (knob is not None and rows == 1) else idx0  # no rows kernel for this plan: arm 1 is arm 0
        log(f"index bytes per cell from the layouts: arm 0 {idx0:.1f}, arm 1 {idx1:.1f}: {(idx0 - idx1) * mesh.ncells / 1e6:.1f} MB less per launch")
        res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, 200) * 1e3, warm=100, alternate=True)  # us
        set_arm(1)
        for arm, v in res.items():
            st = measure.stats(v)
            log(f"  {arm}: median {st.median:8.2f} us  spread {st.spread:5.2f} us  rounds " + " ".join(f"{t:.2f}" for t in v))
        log("  " + measure.verdict_line("arm 0", res["arm 0"], "arm 1", res["arm 1"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
