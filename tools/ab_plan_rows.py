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
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="4:54", help="P:cells-per-direction")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ab_plan_rows.log"))
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("at least 7 rounds")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, gll, ops, lib, pre = (fusgpu_loader.submodule(m) for m in ("boxmesh", "gll", "operators", "_lib", "precompute"))
    knob = getattr(lib, "TUNE_PLAN_ROWS", None)
    clib = lib.load()
    log(f"# tools/ab_plan_rows.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M:%S')}, "
        f"library {clib.fus_source_hash().decode() if hasattr(clib, 'fus_source_hash') else '?'}"
        + ("" if knob is not None else "  (no TUNE_PLAN_ROWS in this tree: both arms run stiffness_plan_kernel)"))
    P, N = (int(v) for v in a.config.split(":"))
    n = P + 1
    mesh = boxmesh.BoxMesh(P, N, perturb=0.16, seed=0)
    pts, wts, D = gll.tabulate_1d(P, np.float64)
    d = torch.device("cuda", 0)
    dm, xd, xg = (torch.from_numpy(np.ascontiguousarray(v)).to(d) for v in (mesh.dofmap, mesh.x_dofs, mesh.x_g))
    G = torch.empty((mesh.ncells, n**3, 6), dtype=torch.float64, device=d)
    pre.compute_scaled_geometrical_factor_device(
        G, (xd, xg), mesh.ncells, torch.from_numpy(pre.tabulate_hex_p1_gradients(gll.tensor_points_3d(pts))).to(d),
        torch.from_numpy(gll.tensor_weights_3d(wts)).to(d))
    x = torch.rand(mesh.ndofs, dtype=torch.float64, device=d)
    cc = 0.5 + torch.rand(mesh.ncells, dtype=torch.float64, device=d)
    y = torch.zeros(mesh.ndofs, dtype=torch.float64, device=d)
    op = ops.stiffness_operator(P, D.flatten(), np.float64)

    def set_arm(v):
        if knob is not None:
            lib.set_tuning(knob, v)

    def one():
        op(x, cc, y, G, dm)

    # same result from both arms (one apply each into a zeroed y), before anything is timed
    ys = []
    for arm in (0, 1):
        set_arm(arm)
        y.zero_()
        one()
        ys.append(y.clone())
    diff = float((ys[0] - ys[1]).abs().max() / ys[0].abs().max())
    (ws, _, epb), = [v for k, v in ops._PLANS._plans.items() if k[-1] != "strips"]
    hdr = ws[:256].cpu().numpy().view(np.int64)
    rows, stride = int(hdr[8]), int(hdr[9])
    log(f"P={P} {N}^3 fp64: {mesh.ncells} cells, {mesh.ndofs} dofs, plan {ws.numel() / 1e6:.1f} MB, rows_consecutive {rows}, run_stride {stride}, "
        f"max |y1 - y0| / max |y0| = {diff:.2e}")
    idx0 = 2 * n**3 + 1024 / epb
    idx1 = 2 * n**2 + 8 * stride / epb if (knob is not None and rows == 1) else idx0  # no rows kernel for this plan: arm 1 is arm 0
    log(f"index bytes per cell from the layouts: arm 0 {idx0:.1f}, arm 1 {idx1:.1f}: {(idx0 - idx1) * mesh.ncells / 1e6:.1f} MB less per launch")

    def ev_time(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            one()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / reps * 1e3  # us

    res = {0: [], 1: []}
    for arm in (0, 1):
        set_arm(arm)
        for _ in range(100):
            one()
    for r in range(a.rounds):
        for arm in ((0, 1) if r % 2 == 0 else (1, 0)):
            set_arm(arm)
            res[arm].append(ev_time(200))
    set_arm(1)
    med, spread = {}, {}
    for arm in (0, 1):
        v = sorted(res[arm])
        med[arm], spread[arm] = v[len(v) // 2], v[-1] - v[0]
        log(f"  arm {arm}: median {med[arm]:8.2f} us  spread {spread[arm]:5.2f} us  rounds " + " ".join(f"{t:.2f}" for t in res[arm]))
    gain, bar = med[0] - med[1], 3 * max(spread.values())
    log(f"  arm 0 - arm 1 = {gain:+.2f} us ({100 * gain / med[0]:+.2f} %); bar: 3 x the larger spread = {bar:.2f} us -> "
        + ("FASTER" if gain > bar else "NOT distinguishable as faster"))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
