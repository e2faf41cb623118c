#!/usr/bin/env python3
"""The shock-capturing sensor and what it costs a Westervelt step, on one MI355X (csrc/modal_sensor.hpp, shock_capture.py),
at config 3 (P = 4, 54^3 cells) and at P = 6 on 36^3 cells -- both 217^3 = 10.2 M dofs -- in fp64 and fp32:

  (a) the sensor launch alone, alternating in the same run with one stiffness apply of the solver (``stiffness_plan_geom_kernel``: the
      gather, the geometry, the contractions and the scatter), and against its own gather traffic: the dofmap (4 bytes per local dof)
      and every dof of the field once;
  (b) the fused Westervelt step plain, with the attachment at every = 1 and at every = 4, interleaved; the baseline is the plain step of
      the same run (no existing kernel changed: that is the step of the code before).

    python tools/time_shock_capture.py [--parts ab] [--log profiles/time_shock_capture.log]

Times: HIP events around back-to-back launches (a); wall clock around synchronised calls (b)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)

CONFIGS = ((4, 54), (6, 36))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_shock_capture.log"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32, help="steps per timed round of (b): a multiple of 4")
    a = ap.parse_args(argv)
    with measure.Log("time_shock_capture", a.log) as log:
        run(a, log)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, nl, sc = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "nonlinear_solver", "shock_capture"))
    log.header()
    L = 0.12
    for P, N in CONFIGS:
        for dt_np in (np.float64, np.float32):
            mesh = boxmesh.BoxMesh(P, N, length=L, perturb=0.16, seed=0, dtype=dt_np)
            h = ls.time_step_parameters(mesh, P, 1480.0, 1.1e6, L)
            dt, _, _ = ls.snap_time_step(h, P, 1480.0, 1.1e6, L)
            name = f"P={P}, {N}^3, {np.dtype(dt_np).name}"
            cap = sc.ShockCapture()
            solver = nl.WesterveltSpectral3D(mesh, dt_np, fused=True, shock_capture=cap)
            solver.init()
            solver.rk4(0.0, 1.0, dt, max_steps=3)
            if "a" in a.parts:
                u, y = solver.u0, torch.zeros_like(solver.b)
                op, cc, G, dofmap = solver._stiffness_operator()
                arms = {"stiffness apply": lambda: op(u, cc, y, G, dofmap), "sensor launch": lambda: cap.launch(u)}
                res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, 100), warm=20)
                ts = np.dtype(dt_np).itemsize
                traffic = mesh.ncells * (P + 1) ** 3 * 4 + mesh.ndofs * ts
                ms, mk = measure.stats(res["sensor launch"]), measure.stats(res["stiffness apply"])
                log(f"(a) {name}: sensor launch {ms.median * 1e3:.1f} us (min {ms.min * 1e3:.1f}, max {ms.max * 1e3:.1f}), stiffness apply "
                    f"{mk.median * 1e3:.1f} us -> {ms.median / mk.median:.3f} x the apply; gather traffic {traffic / 1e6:.1f} MB = "
                    f"{traffic / (ms.median * 1e-3) / 1e12:.2f} TB/s")
            if "b" in a.parts:
                K, t = a.steps, 3 * dt

                def steps(attachment, every):
                    def go():
                        nonlocal t
                        solver.shock_capture, cap.every = attachment, every
                        t, _ = solver.rk4(t, 1.0, dt, max_steps=K)

                    return go

                arms = {"plain": steps(None, 1), "every 1": steps(cap, 1), "every 4": steps(cap, 4)}
                for arm in arms.values():
                    arm()
                res = measure.interleave(arms, a.rounds, lambda fn: measure.host_time(fn, K))
                mp = measure.stats(res["plain"]).median
                log(f"(b) fused Westervelt step ({name}) over {K} steps per round, interleaved:")
                for arm, v in res.items():
                    md = measure.stats(v).median
                    log(f"  {arm:8s} {md:.4f} ms/step  (rounds {', '.join(f'{x:.4f}' for x in v)})  -> {md / mp:.4f} x plain")
                for line in measure.verdict_lines(res, to_us=1e3):
                    log(line)
            del solver, cap, mesh
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
