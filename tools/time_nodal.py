#!/usr/bin/env python3
"""The stiffness apply with a nodal coefficient on one MI355X (csrc/stiffness_geom_nodal.hpp), fp64, perturbed cells, at
config 3 (P = 4, 54^3) and at P = 6, 36^3:

  (a) four launches alternating in one process on the same mesh (tools/measure.py: 100 untimed launches of each, then rounds of 200
      timed launches between one event pair; median of the rounds, verdict at three times the larger spread):
        nodal            stiffness_plan_geom_nodal_kernel: y += K(cc kappa) x, kappa gathered with x, G formed in the kernel
        per-cell         stiffness_plan_geom_kernel: the same launch without the second gather and the coefficient
        two-gather       westervelt_cell_geom_kernel<MASS = false>: the existing pass that gathers two vectors with in-kernel geometry
        pre-scaled G     the general-G kernel on nodal_medium.scale_G(G, kappa, dofmap): the route the nodal kernel replaces
                         (the same operator; it streams 6 n^3 values of G per cell)
      Before anything is timed, nodal and pre-scaled G are checked to agree.
  (b) the fused linear step with and without ``nodal_medium=`` (P = 4, 54^3, G formed in the kernel in both), interleaved.

    python tools/time_nodal.py [--configs 4:54,6:36] [--parts ab] [--log profiles/time_nodal.log]

The comparison that decides the solver's default is nodal against pre-scaled G.  That the nodal launch costs about what the two-gather
pass costs is an expectation this tool checks, not a result it assumes."""
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
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_nodal.log"))
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    import torch

    import fusgpu_loader
    import measure

    torch.cuda.set_device(0)
    boxmesh, ls, nm, ops = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "nodal_medium", "operators"))
    with measure.Log("time_nodal", a.log) as log:
        log.header()
        if "a" in a.parts:
            log(f"(a) one launch, fp64, perturbed cells: event pair around 200 launches after 100 untimed, median of {a.rounds} rounds, "
                "the four kernels alternating")
            for cfg in a.configs.split(","):
                P, N = (int(v) for v in cfg.split(":"))
                pb = measure.device_problem(P, N, np.float64, G=True)
                mesh, dm, x, cc, y = pb.mesh, pb.dm, pb.x, pb.cc, pb.y
                kappa = 1.0 + 2.0 * torch.rand(mesh.ndofs, dtype=pb.tdt, device=pb.dev)  # 3 : 1
                v = torch.rand(mesh.ndofs, dtype=pb.tdt, device=pb.dev)
                geometry = (mesh.x_dofs, mesh.x_g, pb.pts, pb.wts)
                Df = pb.D.flatten()
                nodal = ops.stiffness_operator(P, Df, np.float64, geometry=geometry, nodal=kappa)
                cell = ops.stiffness_operator(P, Df, np.float64, geometry=geometry)
                two = ops.westervelt_cell_operator(P, Df, np.float64, geometry=(mesh.x_g, pb.pts, pb.wts))
                general = ops.stiffness_operator(P, Df, np.float64)
                Gs = nm.scale_G(pb.G, kappa, dm)
                pb.G = None  # (the unscaled array is not read again)
                torch.cuda.empty_cache()
                arms = {"pre-scaled G": lambda: general(x, cc, y, Gs, dm),
                        "nodal": lambda: nodal(x, cc, y, None, dm),
                        "per-cell": lambda: cell(x, cc, y, None, dm),
                        "two-gather": lambda: two.stiffness_only(x, v, cc, cc, y, pb.xd, dm)}
                agree = measure.arms_agree({k: arms[k] for k in ("pre-scaled G", "nodal")}, y)
                log(f"  P={P} {N}^3: {mesh.ncells} cells, {mesh.ndofs} dofs, G' {Gs.numel() * 8 / 1e6:.0f} MB; nodal against pre-scaled G: "
                    f"max |dy| / max |y| = {agree:.2e}")
                if not agree < 1e-11:
                    raise SystemExit("the nodal kernel and the pre-scaled route disagree: nothing is timed")
                y.zero_()
                res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
                med = {k: measure.stats(t).median for k, t in res.items()}
                for name, t in res.items():
                    st = measure.stats(t)
                    log(f"    {name:13s} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f}, spread {st.spread * 1e3:.2f})  "
                        f"= {st.median / med['nodal']:.3f} x nodal")
                log(f"    ratios: nodal / pre-scaled G = {med['nodal'] / med['pre-scaled G']:.3f}, nodal / per-cell = {med['nodal'] / med['per-cell']:.3f}, "
                    f"nodal / two-gather = {med['nodal'] / med['two-gather']:.3f}")
                for line in measure.verdict_lines(res, to_us=1e3, indent="    "):  # every arm against the first: the route the kernel replaces
                    log(line)
                del arms, nodal, cell, two, general, Gs, kappa, v, x, cc, y, dm, pb
                ops._PLANS.clear()
                torch.cuda.empty_cache()

        if "b" in a.parts:
            K, P, N, L = 20, 4, 54, 0.12
            log(f"(b) fused linear steps (P={P}, {N}^3 perturbed cells, fp64, G formed in the kernel), {K} steps per round, interleaved: the "
                "scalar medium (per-cell kernel) and a nodal medium (nodal kernel, nodal lumped mass)")
            mesh = boxmesh.BoxMesh(P, N, length=L, perturb=0.16, seed=0)
            dt, _, _ = ls.snap_time_step(ls.time_step_parameters(mesh, P, 1800.0, 0.5e6, L), P, 1800.0, 0.5e6, L)
            centre = 0.5 * np.asarray(mesh.length)
            bump = lambda xyz: np.exp(-np.sum((xyz - centre) ** 2, axis=1) / (L / 6.0) ** 2)  # noqa: E731
            medium = nm.NodalMedium(lambda xyz: 1500.0 + 300.0 * bump(xyz), lambda xyz: 1000.0 + 200.0 * bump(xyz))
            solvers = {"per-cell": ls.LinearSpectral3D(mesh, np.float64, fused=True, in_kernel_geometry=True),
                       "nodal": ls.LinearSpectral3D(mesh, np.float64, fused=True, nodal_medium=medium)}
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
                log(f"  {name:9s} {m:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in t)})  -> {m / base:.4f} x, {(m - base) * 1e3:+.0f} us per step (4 launches)")
            for line in measure.verdict_lines(res, to_us=1e3):
                log(line)


if __name__ == "__main__":
    main()
