#!/usr/bin/env python3
"""Point sources and element receivers on one MI355X (csrc/point_source.hpp, csrc/element_receive.hpp), at config 3's size
(P = 4, 54^3 perturbed cells: 217^3 = 10.2 M dofs), a 16 x 16-element array on the source face and one point source:

  (a) the fused linear step as it is, with the point source (one more launch per stage), with the receivers recorded after every step
      (one more launch per step), and with both, interleaved in one run;
  (b) each launch alone: ``point_source_kernel`` (1 point) and ``element_receive_kernel`` (256 elements, and one element holding the
      whole face), fp64 and fp32.

    python tools/time_receivers.py [--parts ab] [--elements 16] [--log profiles/time_receivers.log]

Times: wall clock around synchronised ``rk4`` calls (a); HIP events around back-to-back launches (b)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--elements", type=int, default=16, help="elements per direction of the array")
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--mesh-cells", type=int, default=54)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_receivers.log"))
    a = ap.parse_args(argv)
    with measure.Log("time_receivers", a.log) as log:
        run(a, log)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, src, rxm, ops = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "sources", "receivers", "operators"))
    log.header()
    P, N, L, c0, f0, ne = a.degree, a.mesh_cells, 0.12, 1500.0, 0.5e6, a.elements
    mesh = boxmesh.BoxMesh(P, N, length=L, perturb=0.16, seed=0)
    h = ls.time_step_parameters(mesh, P, c0, f0, L)
    dt, _, _ = ls.snap_time_step(h, P, c0, f0, L)
    grid = src.grid_elements(ne, ne, (0.0, L), (0.0, L))
    points = src.PointSources([[0.071, 0.052, 0.063]])
    log(f"P = {P}, {N}^3 cells, {mesh.nlocal} dofs; {ne} x {ne} elements on the source face, 1 point source")

    if "a" in a.parts:
        K = a.steps
        log(f"(a) fused linear step (fp64) over {K} steps, interleaved, {a.rounds} rounds")
        solvers = {"plain": ls.LinearSpectral3D(mesh, np.float64, fused=True), "point": ls.LinearSpectral3D(mesh, np.float64, fused=True, point_source=points)}
        solvers["receivers"], solvers["both"] = solvers["plain"], solvers["point"]
        rx = rxm.ElementReceivers(mesh, grid, np.float64, harmonics=(1,), frequency=f0, n_elements=ne * ne, detJ=solvers["plain"].detJ_f1)
        log(f"  receivers: {int(rx.offsets[-1])} facet-dof entries in {ne * ne} elements")
        clock = {}
        for name in ("plain", "point"):
            solvers[name].init()
            clock[name], _ = solvers[name].rk4(0.0, 1.0, dt, max_steps=3, receivers=rx)
        clock["receivers"], clock["both"] = clock["plain"], clock["point"]

        def steps(name):
            key = {"receivers": "plain", "both": "point"}.get(name, name)  # the solver (and its clock) the variant steps

            def go():
                clock[key], _ = solvers[name].rk4(clock[key], 1.0, dt, max_steps=K, receivers=rx if name in ("receivers", "both") else None)

            return go

        res = measure.interleave({name: steps(name) for name in solvers}, a.rounds, lambda fn: measure.host_time(fn, K))
        base = measure.stats(res["plain"]).median
        for name in solvers:
            m = measure.stats(res[name]).median
            log(f"  {name:9s} {m:.3f} ms/step  {(m - base) * 1e3:+6.0f} us  (rounds {', '.join(f'{x:.3f}' for x in res[name])})")
        for line in measure.verdict_lines(res, to_us=1e3):
            log(line)
        del solvers, rx
        torch.cuda.empty_cache()

    if "b" in a.parts:
        log(f"(b) each launch alone: event pair around 200 launches after 100 untimed, median of {a.rounds} rounds")
        dev = torch.device("cuda", 0)
        for dt_np in (np.float64, np.float32):
            name = np.dtype(dt_np).name
            m32 = mesh if dt_np == np.float64 else boxmesh.BoxMesh(P, N, length=L, perturb=0.16, seed=0, dtype=dt_np)
            y = torch.zeros(mesh.ndofs, dtype=torch.float64, device=dev).to(dtype=torch.float64 if dt_np == np.float64 else torch.float32)
            u = torch.rand(mesh.ndofs, dtype=torch.float64, device=dev).to(y.dtype)
            bound = src.PointSources(points.points, amplitude=1e-9).bind(m32, dt_np, dev, f0)  # small: y stays finite over the launches
            stage = bound.stage_scalars(9.3 / f0)
            cases = {"point source, 1 point": lambda: ops.point_source_terms(y, bound, stage)}
            for E, fn in ((ne * ne, grid), (1, lambda cen: np.zeros(cen.shape[0], dtype=np.int64))):
                rx = rxm.ElementReceivers(m32, fn, dt_np, capacity=1, harmonics=(1,), frequency=f0, n_elements=E)
                coef = rx.factors.row(1e-6)
                cases[f"receive, {E} element(s), {int(rx.offsets[-1])} entries"] = (
                    lambda rx=rx, coef=coef: ops.element_receive(u, rx._dof, rx._wgt, rx._offsets, rx._rec, 0, rx._hre, rx._him, coef))
            res = measure.interleave(cases, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
            for case in cases:
                st = measure.stats(res[case])
                log(f"  {name} {case:45s} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f})")
            del y, u, bound, cases
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
