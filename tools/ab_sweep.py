#!/usr/bin/env python3
"""A/B in one process of the sweep directions of the general-G planned stiffness apply on one MI355X (csrc/stiffness.hpp: mirror_block,
place_batch; the parity: csrc/plan_registry.hpp; knob ``FUS_TUNE_PLAN_SWEEP``), at config 3 (fp64, P = 4, 54^3 perturbed cells) unless told
otherwise:

    arm fwd   knob 0: every launch walks the batches upwards (the only order before the knob existed)
    arm alt   knob 1: every launch walks the other way than the launch before it on the same plan
    arm bwd   knob 2: every launch walks downwards (direction by itself: expected equal to fwd; only alternation should win)

    python tools/ab_sweep.py [--config 4:54] [--dtype f64] [--rounds 9] [--log profiles/ab_sweep.log]

``--config`` takes several P:N pairs separated by commas (the per-degree sweep at ~10 M dofs: 2:108,3:72,4:54,5:43,6:36,7:31,8:27).
Same operator object, same plan workspace, same x / G / y; the knob is the only thing that changes between the arms.  Method of
tools/ab_xcd_group.py: HIP events around back-to-back launches, 100 untimed launches of each arm, then rounds of 200 timed launches, the
arms alternating (their order within a round alternates as well).  Reported per arm: the median of the round times and their spread
(max - min).  The bar (docs/history.md 3.2): an arm counts as faster only if its median is below arm fwd's by more than THREE times the
larger of the two spreads.  Beside the arms: what the LRU model of the memory-side cache (tools/model_g_residency.py) says the second of
two launches finds of G, upwards-upwards and upwards-downwards.

On a tree without the knob (the parent commit) all three arms run upwards: the run then shows what arms of the same code differ by."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KNOB_OF = {"fwd": 0, "alt": 1, "bwd": 2}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="4:54", help="P:cells-per-direction[,P:cells ...]")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-model", action="store_true", help="skip the CPU model's prediction")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ab_sweep.log"))
    a = ap.parse_args(argv)
    if a.rounds < 7:
        ap.error("at least 7 rounds")
    import torch

    import fusgpu_loader
    import measure

    torch.cuda.set_device(0)
    ops, lib = fusgpu_loader.submodule("operators"), fusgpu_loader.submodule("_lib")
    knob = getattr(lib, "TUNE_PLAN_SWEEP", None)
    dt = np.float64 if a.dtype == "f64" else np.float32
    with measure.Log("ab_sweep", a.log) as log:
        log.header("" if knob is not None else "  (no TUNE_PLAN_SWEEP in this tree: every arm walks upwards, the same code)")
        for config in a.config.split(","):
            P, N = (int(v) for v in config.split(":"))
            pb = measure.device_problem(P, N, dt, G=True)
            mesh = pb.mesh
            op = ops.stiffness_operator(P, pb.D.astype(dt).flatten(), dt)

            def set_arm(arm):
                if knob is not None:
                    lib.set_tuning(knob, KNOB_OF[arm])

            def one():
                op(pb.x, pb.cc, pb.y, pb.G, pb.dm)

            arms = {arm: (lambda arm=arm: set_arm(arm), one) for arm in KNOB_OF}
            diff = measure.arms_agree(arms, pb.y)
            log(f"P={P} {N}^3 {a.dtype}: {mesh.ncells} cells, {mesh.ndofs} dofs, max over the arms of max |y - y_fwd| / max |y_fwd| = {diff:.2e}")
            if not a.no_model:
                import model_g_residency

                # the placement knob's group size if one is set; in auto (-1) the model takes the natural order (at the cache's scale the
                # placement inside a window of 8 g batches moves the figure by a few MB: config 3 191.5 MB natural, 187.2 MB with g = 32)
                group = max(lib.get_tuning(lib.TUNE_PLAN_XCD_GROUP) if hasattr(lib, "TUNE_PLAN_XCD_GROUP") else 0, 0)
                for line in model_g_residency.lines_of(model_g_residency.model(P, N, np.dtype(dt).itemsize, group)):
                    log("  " + line)
            res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, 200) * 1e3, warm=100, alternate=True)  # us
            if knob is not None:
                lib.set_tuning(knob, -1)
            st = {arm: measure.stats(v) for arm, v in res.items()}
            for arm, v in res.items():
                log(f"  arm {arm:>4}: median {st[arm].median:8.2f} us  spread {st[arm].spread:5.2f} us"
                    + ("" if arm == "fwd" else "  " + measure.verdict_line("fwd", res["fwd"], arm, v)))
                log("            rounds " + " ".join(f"{t:.2f}" for t in v))
            for line in measure.verdict_lines(res):
                log(line)
            if knob is None:
                lo, hi = min(s.median for s in st.values()), max(s.median for s in st.values())
                log(f"  the arms ran the same code: their medians span {hi - lo:.2f} us, the largest spread is {max(s.spread for s in st.values()):.2f} us")
            del pb, op
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
