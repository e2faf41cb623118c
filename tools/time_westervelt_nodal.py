#!/usr/bin/env python3
"""The Westervelt cell pass with nodal coefficients on one MI355X (csrc/westervelt_geom_nodal.hpp), fp64, perturbed cells,
at config 3 (P = 4, 54^3) and at config 5's shape (P = 6, 36^3):

  (a) three cell passes alternating in one process on the same mesh and the same inputs (tools/measure.py: 100 untimed calls of each,
      then rounds of 200 timed calls between one event pair; median of the rounds, verdict at three times the larger spread):
        two launches     stiffness_plan_geom_nodal_kernel twice, K(c3 kappa3) u then K(c4 kappa4) v: the route the new kernel replaces
        fused nodal      westervelt_cell_geom_nodal_kernel: both contractions, one plan read, one backward, one flush
        per-cell floor   westervelt_cell_geom_kernel<MASS = false> with per-cell constants: the price of the coefficients and of the
                         second forward contraction is fused nodal / per-cell floor
      Before anything is timed, two launches and fused nodal are checked to agree.  The verdict of fused nodal against two launches
      decides ``nonlinear_solver.NODAL_CELL_PASS_DEFAULT``.
  (b) the fused Westervelt step with a nodal medium (both cell-pass routes) against the same step with a per-cell medium, G formed in
      the kernel in all three, interleaved, at both shapes.

    python tools/time_westervelt_nodal.py [--configs 4:54,6:36] [--parts ab] [--log profiles/time_westervelt_nodal.log]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="4:54,6:36", help="P:cells-per-direction, comma separated")
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_westervelt_nodal.log"))
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    import torch

    import fusgpu_loader
    import measure

    torch.cuda.set_device(0)
    boxmesh, ls, nls, nm, ops = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "nonlinear_solver", "nodal_medium", "operators"))
    configs = [tuple(int(v) for v in cfg.split(":")) for cfg in a.configs.split(",")]
    with measure.Log("time_westervelt_nodal", a.log) as log:
        log.header()
        if "a" in a.parts:
            log(f"(a) one cell pass, fp64, perturbed cells: event pair around 200 calls after 100 untimed, median of {a.rounds} rounds, "
                "the three passes alternating")
            for P, N in configs:
                pb = measure.device_problem(P, N, np.float64)
                mesh, dm, u, c3, y = pb.mesh, pb.dm, pb.x, pb.cc, pb.y
                gen = torch.Generator(device=pb.dev).manual_seed(1)
                rnd = lambda n: torch.rand(n, dtype=pb.tdt, device=pb.dev, generator=gen)  # noqa: E731
                kappa3, kappa4 = 1.0 + 2.0 * rnd(mesh.ndofs), 1.0 + 2.0 * rnd(mesh.ndofs)  # 3 : 1 each, different
                v, c4 = rnd(mesh.ndofs), 0.5 + rnd(mesh.ncells)
                geometry = (mesh.x_dofs, mesh.x_g, pb.pts, pb.wts)
                Df = pb.D.flatten()
                n3 = ops.stiffness_operator(P, Df, np.float64, geometry=geometry, nodal=kappa3)
                n4 = ops.stiffness_operator(P, Df, np.float64, geometry=geometry, nodal=kappa4)
                fused = ops.westervelt_cell_operator(P, Df, np.float64, geometry=geometry[1:], nodal=(kappa3, kappa4))
                floor = ops.westervelt_cell_operator(P, Df, np.float64, geometry=geometry[1:])

                def two_launches():
                    n3(u, c3, y, None, dm)
                    n4(v, c4, y, None, dm)

                arms = {"two launches": two_launches,
                        "fused nodal": lambda: fused.stiffness_only(u, v, c3, c4, y, pb.xd, dm),
                        "per-cell floor": lambda: floor.stiffness_only(u, v, c3, c4, y, pb.xd, dm)}
                agree = measure.arms_agree({k: arms[k] for k in ("two launches", "fused nodal")}, y)
                log(f"  P={P} {N}^3: {mesh.ncells} cells, {mesh.ndofs} dofs; fused nodal against two launches: max |db| / max |b| = {agree:.2e}")
                if not agree < 1e-11:
                    raise SystemExit("the fused nodal pass and the two-launch route disagree: nothing is timed")
                y.zero_()
                res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
                med = {k: measure.stats(t).median for k, t in res.items()}
                for name, t in res.items():
                    st = measure.stats(t)
                    log(f"    {name:15s} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f}, spread {st.spread * 1e3:.2f})  "
                        f"= {st.median / med['fused nodal']:.3f} x fused nodal")
                log(f"    ratios: fused nodal / two launches = {med['fused nodal'] / med['two launches']:.3f}, "
                    f"fused nodal / per-cell floor = {med['fused nodal'] / med['per-cell floor']:.3f}")
                for line in measure.verdict_lines(res, to_us=1e3, indent="    "):  # every arm against the first: the route the kernel replaces
                    log(line)
                del arms, n3, n4, fused, floor, kappa3, kappa4, u, v, c3, c4, y, dm, pb
                ops._PLANS.clear()
                torch.cuda.empty_cache()

        if "b" in a.parts:
            K, L = 10, 0.12
            for P, N in configs:
                log(f"(b) fused Westervelt steps (P={P}, {N}^3 perturbed cells, fp64, G formed in the kernel), {K} steps per round, interleaved: a "
                    "per-cell medium (two-gather pass) and a nodal medium through the fused nodal pass and through two launches")
                mesh = boxmesh.BoxMesh(P, N, length=L, perturb=0.16, seed=0)
                dt, _, _ = ls.snap_time_step(ls.time_step_parameters(mesh, P, 1800.0, 0.5e6, L), P, 1800.0, 0.5e6, L)
                centre = 0.5 * np.asarray(mesh.length)
                bump = lambda xyz: np.exp(-np.sum((xyz - centre) ** 2, axis=1) / (L / 6.0) ** 2)  # noqa: E731
                medium = nm.NodalMedium(lambda xyz: 1500.0 + 300.0 * bump(xyz), lambda xyz: 1000.0 + 200.0 * bump(xyz),
                                        nonlinear_coefficient=lambda xyz: 3.5 + 1.5 * bump(xyz),
                                        attenuation_coefficient_dB=lambda xyz: 0.2 + 5.0 * bump(xyz))
                kw = dict(source_frequency=0.5e6, fused=True)
                solvers = {"per-cell": nls.WesterveltSpectral3D(mesh, np.float64, speed_of_sound=1500.0, in_kernel_geometry=True, **kw),
                           "nodal fused": nls.WesterveltSpectral3D(mesh, np.float64, nodal_medium=medium, nodal_cell_pass="fused", **kw),
                           "nodal two-launch": nls.WesterveltSpectral3D(mesh, np.float64, nodal_medium=medium, nodal_cell_pass="two-launch", **kw)}
                clock = {}
                for name, s in solvers.items():
                    s.init()
                    clock[name], _ = s.rk4(0.0, 1.0, dt, max_steps=3)

                def steps(name):
                    clock[name], _ = solvers[name].rk4(clock[name], 1.0, dt, max_steps=K)

                res = measure.interleave({name: (lambda name=name: steps(name)) for name in solvers}, a.rounds, lambda fn: measure.host_time(fn, K))
                base = measure.stats(res["per-cell"]).median
                for name, t in res.items():
                    m = measure.stats(t).median
                    log(f"  {name:16s} {m:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in t)})  -> {m / base:.4f} x, {(m - base) * 1e3:+.0f} us per step (4 cell passes)")
                for line in measure.verdict_lines(res, to_us=1e3):
                    log(line)
                del solvers, mesh
                ops._PLANS.clear()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
