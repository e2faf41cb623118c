#!/usr/bin/env python3
"""Phased-array sources on one MI355X (csrc/source_array.hpp): config 3 (linear, P = 4, 54^3 perturbed cells, fp64,
fused) with four sources, interleaved round by round:

    scalar      source=None: the facet terms of today's scalar waveform (facet_terms_kernel)
    1 element   a one-element SourceArray (facet_source_array_kernel, same field)
    256, 1024   16 x 16 and 32 x 32 elements on the x = 0 face, focusing delays (every facet on the ramp or the plateau)

  (a) the facet launch alone (source set + absorbing set, event pair around 200 launches, median of rounds);
  (b) the step: rk4 over 20 steps.

One solver serves all four: its ``source`` is swapped between arrays bound to its own source-facet tensors (what the
constructor's ``source=`` binds), so the cell launches, the plans and the memory placement are the same in every case.

    python tools/time_sources.py [--parts ab] [--log profiles/time_sources.log]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_sources.py --parts a     # the kernels by name"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_sources.log"))
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, src, ops = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "sources", "operators"))
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# tools/time_sources.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d %H:%M:%S')}")
    L, P, c0, f0 = 0.12, 4, 1500.0, 0.5e6
    mesh = boxmesh.BoxMesh(P, 54, length=L, perturb=0.16, seed=0)
    h = ls.time_step_parameters(mesh, P, c0, f0, L)
    dt, tf, _ = ls.snap_time_step(h, P, c0, f0, L)
    solver = ls.LinearSpectral3D(mesh, np.float64)
    solver.init()
    bd1 = mesh.boundary_facets([getattr(mesh, "source_tag", 2)])
    focus = np.array([0.5 * L, 0.5 * L, 0.5 * L])

    def bind(arr):
        return arr.bind(mesh, bd1, np.float64, solver.dev, frequency=solver.f0, scale=solver.p0 * solver.w0 / solver.c0,
                        coeff1=solver.facet_coeff1, detJ=solver.detJ_f1, dofmap=solver.fdm1)

    def grid(n):
        cen = src.grid_centres(n, n, 0.0, (0.0, L), (0.0, L))
        return src.SourceArray(src.grid_elements(n, n, (0.0, L), (0.0, L)), delay=src.focus_delays(cen, focus, c0), n_elements=n * n)

    cases = {"scalar": None, "1 element": bind(src.SourceArray(lambda c: np.zeros(len(c), np.int64), n_elements=1)),
             "256 elements": bind(grid(16)), "1024 elements": bind(grid(32))}
    log(f"config 3: P={P}, 54^3 perturbed cells, {mesh.ndofs} dofs, fp64, fused; {bd1.shape[0]} source facets, dt {dt:.4e} s")

    def ev_time(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / reps

    t_stage = 30.0 / f0  # every element past its delay: the ramp / plateau branch of the kernel
    if "a" in a.parts:
        log("(a) the facet launch alone (source + absorbing sets in one launch), event pair around 200 launches, median of rounds")
        field = (solver.v, solver.facet_coeff2, solver.detJ_f2, solver.fdm2)
        b = solver.b

        def launch(kind):
            ba = cases[kind]
            if ba is None:
                return lambda: ops.facet_terms(b, (solver.facet_coeff1, solver.source_value(t_stage), None, 0.0, solver.detJ_f1, solver.fdm1),
                                               field)
            stage = ba.stage_scalars(t_stage)
            return lambda: ops.facet_source_terms(b, ba, field, stage=stage)

        fns = {k: launch(k) for k in cases}
        for f in fns.values():
            for _ in range(20):
                f()
        res = {k: [] for k in cases}
        for _ in range(a.rounds):
            for k, f in fns.items():
                res[k].append(ev_time(f, 200) * 1e3)
        for k, v in res.items():
            log(f"  {k:14s} {np.median(v):6.2f} us per launch  (rounds {', '.join(f'{x:.2f}' for x in v)})")

    if "b" in a.parts:
        K = 20
        log(f"(b) the step: rk4 over {K} steps per case, the cases interleaved round by round")
        solver.rk4(0.0, tf, dt, max_steps=3)
        t = t_stage
        res = {k: [] for k in cases}
        for _ in range(a.rounds):
            for k, ba in cases.items():
                solver.source = ba
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t, _ = solver.rk4(t, tf * 100, dt, max_steps=K)
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) / K * 1e3)
        solver.source = None
        base = np.median(res["scalar"])
        for k, v in res.items():
            log(f"  {k:14s} {np.median(v):.4f} ms/step  (rounds {', '.join(f'{x:.4f}' for x in v)})  -> {np.median(v) / base:.4f} x scalar")

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
