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
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="4:54", help="P:cells-per-direction")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--groups", default="8,16,32,64")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-model", action="store_true", help="skip the CPU model's prediction")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ab_xcd_group.log"))
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
    knob = getattr(lib, "TUNE_PLAN_XCD_GROUP", None)
    clib = lib.load()
    log(f"# tools/ab_xcd_group.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M:%S')}, "
        f"library {clib.fus_source_hash().decode() if hasattr(clib, 'fus_source_hash') else '?'}"
        + ("" if knob is not None else "  (no TUNE_PLAN_XCD_GROUP in this tree: every g arm runs the natural order, the same code)"))
    P, N = (int(v) for v in a.config.split(":"))
    n = P + 1
    dt, tdt = (np.float64, torch.float64) if a.dtype == "f64" else (np.float32, torch.float32)
    mesh = boxmesh.BoxMesh(P, N, perturb=0.16, seed=0)
    pts, wts, D = gll.tabulate_1d(P, np.float64)
    d = torch.device("cuda", 0)
    dm, xd, xg = (torch.from_numpy(np.ascontiguousarray(v)).to(d) for v in (mesh.dofmap, mesh.x_dofs, mesh.x_g))
    G = torch.empty((mesh.ncells, n**3, 6), dtype=torch.float64, device=d)
    pre.compute_scaled_geometrical_factor_device(
        G, (xd, xg), mesh.ncells, torch.from_numpy(pre.tabulate_hex_p1_gradients(gll.tensor_points_3d(pts))).to(d),
        torch.from_numpy(gll.tensor_weights_3d(wts)).to(d))
    G = G.to(tdt)
    x = torch.rand(mesh.ndofs, dtype=tdt, device=d)
    cc = 0.5 + torch.rand(mesh.ncells, dtype=tdt, device=d)
    y = torch.zeros(mesh.ndofs, dtype=tdt, device=d)
    op = ops.stiffness_operator(P, D.astype(dt).flatten(), dt)

    arms = ["g0"] + [f"g{int(g)}" for g in a.groups.split(",")] + ["chunks"]

    def set_arm(arm):
        lib.set_tuning(lib.TUNE_XCD_REMAP, 1 if arm == "chunks" else 0)
        if knob is not None:
            lib.set_tuning(knob, 0 if arm == "chunks" else int(arm[1:]))

    def restore():
        lib.set_tuning(lib.TUNE_XCD_REMAP, 0)
        if knob is not None:
            lib.set_tuning(knob, -1)

    def one():
        op(x, cc, y, G, dm)

    # same result from every arm (one apply each into a zeroed y), before anything is timed
    ys = {}
    for arm in arms:
        set_arm(arm)
        y.zero_()
        one()
        ys[arm] = y.clone()
    diff = max(float((ys[arm] - ys["g0"]).abs().max() / ys["g0"].abs().max()) for arm in arms)
    log(f"P={P} {N}^3 {a.dtype}: {mesh.ncells} cells, {mesh.ndofs} dofs, max over the arms of max |y - y_g0| / max |y_g0| = {diff:.2e}")
    pred = {}
    if not a.no_model:
        import model_x_fetch

        r = model_x_fetch.model(P, N, [1] + [int(g) for g in a.groups.split(",")], 48, np.dtype(dt).itemsize)
        pred = {("g0" if g == 1 else f"g{g}"): mb for g, mb in r["mb"].items() if g != "chunks"}
        pred["chunks"] = r["mb"]["chunks"]
        log(f"model (tools/model_x_fetch.py, W = 48): {r['nbatch']} batches, touches per dof {r['touches_per_dof']:.3f}, x once {r['floor_mb']:.1f} MB")

    def ev_time(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            one()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / reps * 1e3  # us

    res = {arm: [] for arm in arms}
    for arm in arms:
        set_arm(arm)
        for _ in range(100):
            one()
    for r in range(a.rounds):
        for arm in (arms if r % 2 == 0 else arms[::-1]):
            set_arm(arm)
            res[arm].append(ev_time(200))
    restore()
    med, spread = {}, {}
    for arm in arms:
        v = sorted(res[arm])
        med[arm], spread[arm] = v[len(v) // 2], v[-1] - v[0]
    for arm in arms:
        gain, bar = med["g0"] - med[arm], 3 * max(spread["g0"], spread[arm])
        verdict = "" if arm == "g0" else (f"  g0 - arm = {gain:+6.2f} us ({100 * gain / med['g0']:+.2f} %), bar {bar:.2f} us -> "
                                          + ("FASTER" if gain > bar else "SLOWER" if -gain > bar else "not distinguishable"))
        log(f"  arm {arm:>6}: median {med[arm]:8.2f} us  spread {spread[arm]:5.2f} us"
            + (f"  model x fetch {pred[arm]:6.1f} MB" if arm in pred else "") + verdict)
        log("              rounds " + " ".join(f"{t:.2f}" for t in res[arm]))
    if knob is None:
        g_arms = [arm for arm in arms if arm != "chunks"]
        lo, hi = min(med[arm] for arm in g_arms), max(med[arm] for arm in g_arms)
        log(f"  the g arms ran the same code: their medians span {hi - lo:.2f} us, the largest spread is {max(spread[arm] for arm in g_arms):.2f} us")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
