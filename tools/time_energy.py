#!/usr/bin/env python3
"""The reduction kernel and what is built on it, on one MI355X (csrc/reduce.hpp, diagnostics.py), at config 3 (P = 4,
54^3 cells, fp64) and at P = 6 on 36^3 cells -- both 217^3 = 10.2 M dofs:

  (a) the ``reduce_terms`` launch pair alone (``reduce_terms_kernel`` + ``reduce_finish_kernel``) in its three shapes -- dot
      ``(a, b, w)``, energy ``(v, v, m), (u, y), x = u`` and guard ``x = u`` -- fp64 and fp32, as bytes per second of the DISTINCT
      vectors each reads, alternating in the same run with the RK4 stage vector pass (the streaming kernel of the same access shape);
  (b) the fused linear step plain, with ``energy`` at every = 1 and every = 16, and with ``guard`` at every = 64, interleaved; the
      baseline is the plain step of the same run (no existing kernel changed: that is the step of the code before);
  (c) one ``stable_time_step()`` call.

    python tools/time_energy.py [--parts abc] [--log profiles/time_energy.log]

Times: HIP events around back-to-back launch pairs (a); wall clock around synchronised calls (b, c)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)

N_DOFS = 217**3
CONFIGS = ((4, 54), (6, 36))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_energy.log"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64, help="steps per timed round of (b): a multiple of 64, the guard's cadence")
    a = ap.parse_args(argv)
    with measure.Log("time_energy", a.log) as log:
        run(a, log)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, lib, red_mod, diag = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "_lib", "reductions", "diagnostics"))
    log.header()
    L = 0.12

    if "a" in a.parts:
        log(f"(a) one reduce_terms launch pair over {N_DOFS} entries: event pair around 200 pairs after 100 untimed, median of {a.rounds} "
            "rounds, alternating with the RK4 stage vector pass (kind 0, 12 touches)")
        for dt_np in (np.float64, np.float32):
            tdt, ts = lib.torch_dtype(dt_np), np.dtype(dt_np).itemsize
            vec = [torch.randn(N_DOFS, dtype=torch.float64, device="cuda").to(tdt) for _ in range(8)]
            stage = getattr(lib.load(), f"fus_rk4_stage_{lib.suffix(tdt)}")
            red = red_mod.Reducer()
            u, v, m, y = vec[:4]

            def stage_pass():
                lib.check(stage(1e-9, 1e-9, 0, *(x.data_ptr() for x in vec), N_DOFS, N_DOFS, lib.stream_ptr()), "fus_rk4_stage")

            cases = [("rk4 stage pass", 12, stage_pass),
                     ("dot (a, b, w)", 3, lambda: red.terms(sum0=(u, v, m))),
                     ("energy (v, v, m), (u, y), x = u", 4, lambda: red.terms(sum0=(v, v, m), sum1=(u, y, None), x=u)),
                     ("guard x = u", 1, lambda: red.terms(x=u))]
            res = measure.interleave({name: one for name, _, one in cases}, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
            ref = None
            for name, nvec, _ in cases:
                st, nb = measure.stats(res[name]), nvec * N_DOFS * ts
                bw = nb / (st.median * 1e-3) / 1e12
                ref = bw if ref is None else ref
                log(f"  {np.dtype(dt_np).name} {name:34s} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f})  reads "
                    f"{nb / 1e6:7.1f} MB  {bw:.2f} TB/s  = {bw / ref:.3f} x the stage pass")
            del vec, cases, u, v, m, y
            torch.cuda.empty_cache()

    for P, N in CONFIGS if ("b" in a.parts or "c" in a.parts) else ():
        mesh = boxmesh.BoxMesh(P, N, length=L, perturb=0.16, seed=0)
        h = ls.time_step_parameters(mesh, P, 1500.0, 0.5e6, L)
        dt, _, _ = ls.snap_time_step(h, P, 1500.0, 0.5e6, L)
        solver = ls.LinearSpectral3D(mesh, np.float64, fused=True)
        solver.init()
        solver.rk4(0.0, 1.0, dt, max_steps=3)
        if "b" in a.parts:
            K, t = a.steps, 3 * dt
            log(f"(b) fused linear step (P={P}, {N}^3, fp64) over {K} steps per round: plain, energy every 1 / 16, guard every 64, interleaved")
            e1, e16 = diag.EnergyRecorder(solver, every=1, capacity=K), diag.EnergyRecorder(solver, every=16, capacity=K)
            guard = diag.FieldGuard(every=64)

            def steps(**kw):
                def go():
                    nonlocal t
                    t, _ = solver.rk4(t, 1.0, dt, max_steps=K, **kw)

                return go

            arms = {"plain": steps(), "energy every 1": (e1.reset, steps(energy=e1)), "energy every 16": (e16.reset, steps(energy=e16)),
                    "guard every 64": (guard.reset, steps(guard=guard))}
            for arm in arms.values():  # every path once, untimed (the recorder's apply builds no new plan, but loads its kernels)
                measure._arm(arm)[0]()
                measure._arm(arm)[1]()
            res = measure.interleave(arms, a.rounds, lambda fn: measure.host_time(fn, K))
            mp = measure.stats(res["plain"]).median
            for name, v in res.items():
                md = measure.stats(v).median
                per = {"plain": "", "energy every 1": f", +{(md - mp) * 1e3:.0f} us per record", "energy every 16": f", +{(md - mp) * 16e3:.0f} us per record",
                       "guard every 64": f", +{(md - mp) * 64e3:.0f} us per check"}[name]
                log(f"  {name:16s} {md:.4f} ms/step  (rounds {', '.join(f'{x:.4f}' for x in v)})  -> {md / mp:.4f} x plain{per}")
            for line in measure.verdict_lines(res, to_us=1e3):
                log(line)
            tot = e1.energies()[3]
            log(f"  energy of the last round: first {tot[0]:.6e}, last {tot[-1]:.6e} ({len(tot)} records)")
        if "c" in a.parts:
            ms = measure.host_time(lambda: solver.stable_time_step(0.8))
            log(f"(c) stable_time_step() (P={P}, {N}^3, fp64): {ms:.1f} ms; limit {solver.stable_limit:.6e} s (lambda_max {solver.lambda_max:.4e}, "
                f"damping_max {solver.damping_max:.4e}), snapped CFL step {dt:.6e} s = {dt / solver.stable_limit:.3f} x the limit")
        del solver, mesh
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
