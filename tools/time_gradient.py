#!/usr/bin/env python3
"""The gradient cell operator on one MI355X (csrc/gradient_geom.hpp): the launch of ``gradient_plan_geom_kernel`` alone,
alternating in the same run with ``stiffness_plan_geom_kernel`` on the same mesh and the same plan, at config 3 (P = 4, 54^3 perturbed
cells) and at config 5's shape (P = 6, 36^3), fp64 and fp32.

    python tools/time_gradient.py [--configs 4:54,6:36] [--log profiles/time_gradient.log]

Times: HIP events around back-to-back launches (the method of tools/time_bioheat.py): 100 untimed launches of each, then rounds of
200 timed launches, the two kernels alternating; the median over the rounds is reported.

Bytes model (stated, not measured):  ncell (plan bytes + x read) + C y read-modify-write, with per cell
    plan bytes = 2 Nd (slots) + 4 Nd (the batch's dof list; an upper bound where the launch reads the run tables instead)
                 + 32 (x_dofs row) + ts (cell constant)
    x read     = Nd ts (an upper bound: the gather reads each DISTINCT dof of a batch once)
and  y read-modify-write = 2 ts ndofs  per component, C = 3 components for the gradient and 1 for the stiffness apply (Nd = (P + 1)^3,
ts = bytes per scalar).  The vertex coordinates (x_g: 24 B per vertex) stay in cache and are left out.

The expectation written down before the first run: the gradient launch is not slower than the stiffness apply with in-kernel geometry
at the same shape, although it issues 3 x the global atomics and far fewer fp64 instructions."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def model_bytes(P, ncell, ndofs, ts, components):
    Nd = (P + 1) ** 3
    return ncell * (2 * Nd + 4 * Nd + 32 + ts + Nd * ts) + components * 2 * ts * ndofs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4:54,6:36", help="P:cells-per-direction, comma separated")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_gradient.log"))
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    import torch

    import fusgpu_loader
    import measure

    torch.cuda.set_device(0)
    gll, ops, lib = (fusgpu_loader.submodule(m) for m in ("gll", "operators", "_lib"))
    with measure.Log("time_gradient", a.log) as log:
        log.header()
        log(f"one launch, event pair around 200 launches after 100 untimed, median of {a.rounds} rounds, the two kernels alternating; "
            "model: ncell (plan bytes + x read) + C y read-modify-write (see the tool's docstring)")
        for cfg in a.configs.split(","):
            P, N = (int(v) for v in cfg.split(":"))
            pb = measure.device_problem(P, N, np.float64)
            mesh, dm = pb.mesh, pb.dm
            for dt_np in (np.float64, np.float32):
                ts = np.dtype(dt_np).itemsize
                pts, wts, D = gll.tabulate_1d(P, dt_np)
                geometry = (mesh.x_dofs, mesh.x_g, pts, wts)
                tdt = lib.torch_dtype(dt_np)
                x, cc, y = pb.x.to(tdt), pb.cc.to(tdt), pb.y.to(tdt)
                y3 = torch.zeros((3, mesh.ndofs), dtype=tdt, device="cuda")
                stiff = ops.stiffness_operator(P, D.flatten(), dt_np, geometry=geometry)
                grad = ops.gradient_operator(P, D.flatten(), dt_np, geometry=geometry)
                stiff.prepare(dm)
                grad.prepare(dm)  # the same cache entry: one plan for both
                comps = {"stiffness_plan_geom": 1, "gradient_plan_geom": 3}
                arms = {"stiffness_plan_geom": lambda: stiff(x, cc, y, None, dm), "gradient_plan_geom": lambda: grad(x, cc, y3, dm)}
                res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
                base = measure.stats(res["stiffness_plan_geom"]).median
                for name, v in res.items():
                    st = measure.stats(v)
                    nb = model_bytes(P, mesh.ncells, mesh.ndofs, ts, comps[name])
                    log(f"  P={P} {N}^3 {np.dtype(dt_np).name} {name:20s} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f}, spread {st.spread * 1e3:.2f})  "
                        f"model {nb / 1e6:7.1f} MB  {nb / (st.median * 1e-3) / 1e12:.2f} TB/s  = {st.median / base:.3f} x the stiffness apply")
                del x, cc, y, y3, stiff, grad, arms
            ops._PLANS.clear()
            del dm, mesh, pb
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
