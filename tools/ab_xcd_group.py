#!/usr/bin/env python3
"""A/B in one process of the batch placements of the general-G planned stiffness apply on one MI355X (csrc/stiffness.hpp: group_block,
place_batch; knob ``FUS_TUNE_PLAN_XCD_GROUP``), at config 3 (fp64, P = 4, 54^3 perturbed cells) unless told otherwise:

    arm g0       natural order: workgroup b runs batch b, so the batches of an XCD are 8 apart and share no dof of x
    arm g8 ...   g consecutive batches per XCD label (g = 8, 16, 32, 64)
    arm chunks   ``FUS_TUNE_XCD_REMAP`` = 1: one contiguous eighth of the batches per XCD (the old mode)

    python tools/ab_xcd_group.py [--config 4:54] [--dtype f64] [--groups 8,16,32,64] [--rounds 9] [--log profiles/ab_xcd_group.log]

Same operator object, same plan workspace, same x / G / y; the two knobs are the only thing that changes between the arms.  Method of
tools/ab_plan_rows.py: HIP events around back-to-back launches, 100 untimed launches of each arm, then rounds of 200 timed launches, the
arms alternating (their order within a round alternates as well).  Reported per arm: the median of the round times and their spread
(max - min).  The bar (docs/history.md 3.2): an arm counts as faster only if its median is below arm g0's by more than THREE times the
larger of the two spreads.  Beside each arm: the x fetch per launch that tools/model_x_fetch.py predicts for it.

On a tree without the knob (the parent commit) every g arm runs the natural order: the run then shows what arms of the same code differ by."""
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
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--groups", default="8,16,32,64")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-model", action="store_true", help="skip the CPU model's prediction")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ab_xcd_group.log"))
    a = ap.parse_args(argv)
    if a.rounds < 7:
        ap.error("at least 7 rounds")
    import torch

    import fusgpu_loader
    import measure

    torch.cuda.set_device(0)
    ops, lib = fusgpu_loader.submodule("operators"), fusgpu_loader.submodule("_lib")
    knob = getattr(lib, "TUNE_PLAN_XCD_GROUP", None)
    with measure.Log("ab_xcd_group", a.log) as log:
        log.header("" if knob is not None else "  (no TUNE_PLAN_XCD_GROUP in this tree: every g arm runs the natural order, the same code)")
        P, N = (int(v) for v in a.config.split(":"))
        dt = np.float64 if a.dtype == "f64" else np.float32
        pb = measure.device_problem(P, N, dt, G=True)
        mesh = pb.mesh
        op = ops.stiffness_operator(P, pb.D.astype(dt).flatten(), dt)

        def set_arm(arm):
            lib.set_tuning(lib.TUNE_XCD_REMAP, 1 if arm == "chunks" else 0)
            if knob is not None:
                lib.set_tuning(knob, 0 if arm == "chunks" else int(arm[1:]))

        def restore():
            lib.set_tuning(lib.TUNE_XCD_REMAP, 0)
            if knob is not None:
                lib.set_tuning(knob, -1)

        def one():
            op(pb.x, pb.cc, pb.y, pb.G, pb.dm)

        arms = {arm: (lambda arm=arm: set_arm(arm), one) for arm in ["g0"] + [f"g{int(g)}" for g in a.groups.split(",")] + ["chunks"]}
        diff = measure.arms_agree(arms, pb.y)
        log(f"P={P} {N}^3 {a.dtype}: {mesh.ncells} cells, {mesh.ndofs} dofs, max over the arms of max |y - y_g0| / max |y_g0| = {diff:.2e}")
        pred = {}
        if not a.no_model:
            import model_x_fetch

            r = model_x_fetch.model(P, N, [1] + [int(g) for g in a.groups.split(",")], 48, np.dtype(dt).itemsize)
            pred = {("g0" if g == 1 else f"g{g}"): mb for g, mb in r["mb"].items() if g != "chunks"}
            pred["chunks"] = r["mb"]["chunks"]
            log(f"model (tools/model_x_fetch.py, W = 48): {r['nbatch']} batches, touches per dof {r['touches_per_dof']:.3f}, x once {r['floor_mb']:.1f} MB")
        res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, 200) * 1e3, warm=100, alternate=True)  # us
        restore()
        st = {arm: measure.stats(v) for arm, v in res.items()}
        for arm, v in res.items():
            log(f"  arm {arm:>6}: median {st[arm].median:8.2f} us  spread {st[arm].spread:5.2f} us"
                + (f"  model x fetch {pred[arm]:6.1f} MB" if arm in pred else "")
                + ("" if arm == "g0" else "  " + measure.verdict_line("g0", res["g0"], "arm", v)))
            log("              rounds " + " ".join(f"{t:.2f}" for t in v))
        if knob is None:
            g_arms = [arm for arm in arms if arm != "chunks"]
            lo, hi = min(st[arm].median for arm in g_arms), max(st[arm].median for arm in g_arms)
            log(f"  the g arms ran the same code: their medians span {hi - lo:.2f} us, the largest spread is {max(st[arm].spread for arm in g_arms):.2f} us")
    return 0


if __name__ == "__main__":
    sys.exit(main())
