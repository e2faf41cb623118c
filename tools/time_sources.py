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

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_sources.log"))
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args(argv)
    with measure.Log("time_sources", a.log) as log:
        run(a, log)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, src, ops = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "sources", "operators"))
    log.header()
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

        res = measure.interleave({k: launch(k) for k in cases}, a.rounds, lambda fn: measure.event_time(fn, 200) * 1e3, warm=20)  # us
        for k, v in res.items():
            log(f"  {k:14s} {measure.stats(v).median:6.2f} us per launch  (rounds {', '.join(f'{x:.2f}' for x in v)})")
        for line in measure.verdict_lines(res):
            log(line)

    if "b" in a.parts:
        K = 20
        log(f"(b) the step: rk4 over {K} steps per case, the cases interleaved round by round")
        solver.rk4(0.0, tf, dt, max_steps=3)
        t = t_stage

        def steps():
            nonlocal t
            t, _ = solver.rk4(t, tf * 100, dt, max_steps=K)

        res = measure.interleave({k: (lambda ba=ba: setattr(solver, "source", ba), steps) for k, ba in cases.items()}, a.rounds,
                                 lambda fn: measure.host_time(fn, K))
        solver.source = None
        base = measure.stats(res["scalar"]).median
        for k, v in res.items():
            med = measure.stats(v).median
            log(f"  {k:14s} {med:.4f} ms/step  (rounds {', '.join(f'{x:.4f}' for x in v)})  -> {med / base:.4f} x scalar")
        for line in measure.verdict_lines(res, to_us=1e3):
            log(line)


if __name__ == "__main__":
    main()
