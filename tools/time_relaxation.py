#!/usr/bin/env python3
"""Relaxation mechanisms on one MI355X (csrc/relaxation.hpp, relaxation.py), at config 3's size (P = 4, 54^3 cells:
217^3 = 10.2 M dofs, perturbed cells: G formed in the kernel):

  (a) the pass alone (``relax_stage_kernel<T, NR, W, NT, PERDOF>``), NR = 1, 2, 3, MIDDLE (the kind with the most touches) with
      scalar and with per-dof weights, fp64 and fp32, as achieved bytes per second against the touches of csrc/relax_table.hpp,
      alternating in the same run with the wave solvers' stage pass (``rk4_stage_kernel``, kind 0: 12 touches), which has the same
      access shape -- the expectation to test is that the pass streams at that kernel's rate;
  (b) the fused linear step with NR = 2 (scalar weights, and per-cell weights) against the step without mechanisms, interleaved.

    python tools/time_relaxation.py [--parts ab] [--log profiles/time_relaxation.log]

Times: HIP events around back-to-back launches (a); wall clock around synchronised ``rk4`` calls (b)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)

N_DOFS = 217**3


def touches(kind, nr, perdof):
    """csrc/relax_table.hpp relax_touches: u_base, vn, ur and per mechanism 3 (FIRST, LAST) or 5 (MIDDLE) arrays, + 1 with per-dof weights."""
    return 3 + nr * ((5 if kind == 1 else 3) + (1 if perdof else 0))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_relaxation.log"))
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    with measure.Log("time_relaxation", a.log) as log:
        run(a, log)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, rx, ops, lib = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "relaxation", "operators", "_lib"))
    log.header()

    if "a" in a.parts:
        log(f"(a) one launch over {N_DOFS} dofs: event pair around 200 launches after 100 untimed, median of {a.rounds} rounds, "
            "alternating with the RK4 stage vector pass of the wave solvers (kind 0, 12 touches)")
        for dt_np in (np.float64, np.float32):
            tdt, ts = lib.torch_dtype(dt_np), np.dtype(dt_np).itemsize
            vec = [torch.rand(N_DOFS, dtype=torch.float64, device="cuda").to(tdt) for _ in range(8)]
            rk4 = getattr(lib.load(), f"fus_rk4_stage_{lib.suffix(tdt)}")
            stride = -(-N_DOFS // 4) * 4
            state = [torch.rand((3, stride), dtype=torch.float64, device="cuda").to(tdt) * 1e-3 for _ in range(4)]  # xi0 xin acc kappa
            tau = np.array([3e-7, 1e-7, 3e-8])

            def rk4_pass():
                lib.check(rk4(1e-9, 1e-9, 0, *(x.data_ptr() for x in vec), N_DOFS, N_DOFS, lib.stream_ptr()), "fus_rk4_stage")

            def relax_pass(kind, nr, perdof):
                x0, xn, ac, kd = (s[:nr] for s in state)
                ops.relax_stage(1e-9, 1e-9, 1e-9, kind, tau[:nr], kd if perdof else np.full(nr, 1e-3), x0, xn, ac, vec[0], vec[1], vec[2], N_DOFS)

            cases = [("rk4 stage pass", 12 * N_DOFS * ts, rk4_pass)]
            for nr in (1, 2, 3):
                for perdof in (False, True):
                    cases.append((f"relax MIDDLE NR={nr} {'per-dof' if perdof else 'scalar '}", touches(1, nr, perdof) * N_DOFS * ts,
                                  lambda nr=nr, perdof=perdof: relax_pass(1, nr, perdof)))
            cases.append(("relax FIRST  NR=2 scalar ", touches(0, 2, False) * N_DOFS * ts, lambda: relax_pass(0, 2, False)))
            cases.append(("relax LAST   NR=2 scalar ", touches(2, 2, False) * N_DOFS * ts, lambda: relax_pass(2, 2, False)))
            res = measure.interleave({name: one for name, _, one in cases}, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
            ref = None
            for name, nb, _ in cases:
                st = measure.stats(res[name])
                bw = nb / (st.median * 1e-3) / 1e12
                ref = bw if ref is None else ref
                log(f"  {np.dtype(dt_np).name} {name:28s} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f})  model {nb / 1e6:7.1f} MB"
                    f"  {bw:.2f} TB/s  = {bw / ref:.3f} x the rk4 stage pass")
            del vec, state, cases
            torch.cuda.empty_cache()

    if "b" in a.parts:
        K = 20
        log(f"(b) fused linear steps (P=4, 54^3 perturbed cells, fp64, G formed in the kernel), {K} steps per round, interleaved: without "
            "mechanisms, with NR = 2 scalar weights, with NR = 2 per-cell weights")
        mesh = boxmesh.BoxMesh(4, 54, length=0.12, perturb=0.16, seed=0)
        h = ls.time_step_parameters(mesh, 4, 1500.0, 0.5e6, 0.12)
        dt, _, _ = ls.snap_time_step(h, 4, 1500.0, 0.5e6, 0.12)
        fit = rx.fit_power_law(0.5, 1.1, 0.25e6, 2.5e6, n=2, speed_of_sound=1500.0, with_thermoviscous=False)
        log(f"  dt = {dt:.4g} s, tau = {fit.tau}, dt / min(tau) = {dt / fit.tau.min():.3f}")
        percell = np.repeat(fit.kappa[:, None], mesh.ncells, axis=1) * np.random.default_rng(0).uniform(0.5, 1.5, mesh.ncells)
        solvers = {"plain": ls.LinearSpectral3D(mesh, np.float64, fused=True),
                   "NR=2 scalar": ls.LinearSpectral3D(mesh, np.float64, fused=True, relaxation=rx.RelaxationAbsorption(fit.tau, fit.kappa)),
                   "NR=2 per-cell": ls.LinearSpectral3D(mesh, np.float64, fused=True, relaxation=rx.RelaxationAbsorption(fit.tau, percell))}
        clock = {}
        for name, s in solvers.items():
            s.init()
            clock[name], _ = s.rk4(0.0, 1.0, dt, max_steps=3)

        def steps(name):
            clock[name], _ = solvers[name].rk4(clock[name], 1.0, dt, max_steps=K)

        res = measure.interleave({name: (lambda name=name: steps(name)) for name in solvers}, a.rounds, lambda fn: measure.host_time(fn, K))
        base = measure.stats(res["plain"]).median
        for name, v in res.items():
            med = measure.stats(v).median
            log(f"  {name:14s} {med:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in v)})  -> {med / base:.4f} x, {(med - base) * 1e3:+.0f} us per step (4 launches)")
        model = {n_: 4 * 3 + 16 * 2 + (4 * 2 if n_ == "NR=2 per-cell" else 0) for n_ in ("NR=2 scalar", "NR=2 per-cell")}
        for n_, t_ in model.items():
            log(f"  byte model {n_}: {t_} vector touches per step = {t_ * N_DOFS * 8 / 1e6:.0f} MB")
        for line in measure.verdict_lines(res, to_us=1e3):
            log(line)


if __name__ == "__main__":
    main()
