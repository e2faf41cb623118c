#!/usr/bin/env python3
"""Sampled source waveforms on one MI355X (csrc/source_wave.hpp) against the analytic sources they stand beside: config 3
(linear, P = 4, 54^3 perturbed cells, fp64, fused), the arms interleaved round by round, the verdict ``measure.verdict`` of the
waveform arm against the analytic arm of the SAME run (never a fixed number):

  (a) the facet launch alone (source set + absorbing set): 256 elements with focusing delays, analytic
      (facet_source_array_kernel) against a table of R = 256 rows of Nt = 4096 samples (facet_source_wave_kernel);
  (b) the point launch alone, 1 and 1024 points: analytic (point_source_kernel) against the table (point_source_wave_kernel);
  (c) the fused step: rk4 over 20 steps with each of the two arrays.

The table rows are the analytic waveform itself, sampled over 40 periods, so both arms add the same values (to the interpolation
error) and every entry is inside the table at the measured stage time.

    python tools/time_waveform_sources.py [--parts abc] [--log profiles/time_waveform_sources.log]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)

NT = 4096


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_waveform_sources.log"))
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args(argv)
    with measure.Log("time_waveform_sources", a.log) as log:
        run(a, log)


def sampled(src, f0, phase, periods=40.0):
    """The analytic continuous-wave rows ``W(s) cos(w0 s + phi_r)`` over ``periods`` periods, NT samples, with the analytic derivative."""
    dt = periods / f0 / (NT - 1)
    s = np.arange(NT) * dt
    env, denv = src._window(s, f0)
    w0 = 2.0 * np.pi * f0
    arg = w0 * s[None, :] + np.asarray(phase, dtype=np.float64)[:, None]
    return src.SampledWaveform(env * np.cos(arg), dt, derivative=denv * np.cos(arg) - env * w0 * np.sin(arg))


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
    rng = np.random.default_rng(0)
    n, E = 16, 256
    cen = src.grid_centres(n, n, 0.0, (0.0, L), (0.0, L))
    ids, delay, phase = src.grid_elements(n, n, (0.0, L), (0.0, L)), src.focus_delays(cen, focus, c0), rng.uniform(-np.pi, np.pi, E)

    def bind(arr):
        return arr.bind(mesh, bd1, np.float64, solver.dev, frequency=solver.f0, scale=solver.p0 * solver.w0 / solver.c0,
                        coeff1=solver.facet_coeff1, detJ=solver.detJ_f1, dofmap=solver.fdm1)

    arrays = {"analytic": bind(src.SourceArray(ids, phase=phase, delay=delay, n_elements=E)),
              "waveform": bind(src.SourceArray(ids, delay=delay, n_elements=E, waveform=sampled(src, f0, phase)))}
    tab = arrays["waveform"].table
    log(f"config 3: P={P}, 54^3 perturbed cells, {mesh.ndofs} dofs, fp64, fused; {bd1.shape[0]} source facets, {E} elements, dt {dt:.4e} s; "
        f"table {tuple(tab.shape)} fp64 = {tab.numel() * 8 / 2**20:.1f} MiB")
    t_stage = 30.0 / f0  # every element past its delay and inside the table
    b = solver.b

    if "a" in a.parts:
        log("(a) the facet launch alone (source + absorbing sets in one launch), event pair around 200 launches, median of rounds")
        field = (solver.v, solver.facet_coeff2, solver.detJ_f2, solver.fdm2)
        ys = {}
        for k, ba in arrays.items():
            b.zero_()
            ops.facet_source_terms(b, ba, None, stage=ba.stage_scalars(t_stage))
            ys[k] = b.clone()
        b.zero_()
        log(f"  the two arms' source terms differ by {float((ys['waveform'] - ys['analytic']).abs().max() / ys['analytic'].abs().max()):.2e} "
            "of the largest entry (the interpolation error)")

        def launch(ba):
            stage = ba.stage_scalars(t_stage)
            return lambda: ops.facet_source_terms(b, ba, field, stage=stage)

        res = measure.interleave({k: launch(ba) for k, ba in arrays.items()}, a.rounds, lambda fn: measure.event_time(fn, 200) * 1e3, warm=20)
        for k, v in res.items():
            log(f"  {k:10s} {measure.stats(v).median:6.2f} us per launch  (rounds {', '.join(f'{x:.2f}' for x in v)})")
        for line in measure.verdict_lines(res):
            log(line)

    if "b" in a.parts:
        log("(b) the point launch alone, event pair around 200 launches, median of rounds")
        for m in (1, 1024):
            pts = rng.uniform(0.05 * L, 0.95 * L, (m, 3))
            R = min(m, 256)
            ph = rng.uniform(-np.pi, np.pi, m)
            wf = sampled(src, f0, ph[:R])
            arms = {"analytic": src.PointSources(pts, phase=ph), "waveform": src.PointSources(pts, waveform=wf, waveform_of_point=np.arange(m) % R)}
            su = arms["analytic"].setup(mesh)
            bound = {k: ps.bind(mesh, np.float64, solver.dev, f0, setup=su) for k, ps in arms.items()}

            def launch(bp):
                stage = bp.stage_scalars(t_stage)
                return lambda: ops.point_source_terms(b, bp, stage)

            res = measure.interleave({k: launch(bp) for k, bp in bound.items()}, a.rounds, lambda fn: measure.event_time(fn, 200) * 1e3, warm=20)
            for k, v in res.items():
                log(f"  {m:5d} point(s) {k:10s} {measure.stats(v).median:6.2f} us per launch  (rounds {', '.join(f'{x:.2f}' for x in v)})")
            for line in measure.verdict_lines(res):
                log(line)
        b.zero_()

    if "c" in a.parts:
        K = 20
        log(f"(c) the fused step: rk4 over {K} steps per arm, the arms interleaved round by round")
        solver.rk4(0.0, tf, dt, max_steps=3)
        t = t_stage

        def use(ba):
            solver.source = solver._facet_source = ba

        def steps():
            nonlocal t
            t, _ = solver.rk4(t, tf * 100, dt, max_steps=K)
            if t > 36.0 / f0:  # stay inside the table
                t = t_stage

        res = measure.interleave({k: (lambda ba=ba: use(ba), steps) for k, ba in arrays.items()}, a.rounds, lambda fn: measure.host_time(fn, K))
        for k, v in res.items():
            log(f"  {k:10s} {measure.stats(v).median:.4f} ms/step  (rounds {', '.join(f'{x:.4f}' for x in v)})")
        for line in measure.verdict_lines(res, to_us=1e3):
            log(line)


if __name__ == "__main__":
    main()
