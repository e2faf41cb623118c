#!/usr/bin/env python3
"""The Pennes bioheat solver on one MI355X (csrc/bioheat.hpp, bioheat.py), at config 3's size (P = 4, 54^3 cells:
217^3 = 10.2 M dofs, perturbed cells: G formed in the kernel):

  (a) the stage kernel alone (``bioheat_stage_kernel<T, W, NT>``), FIRST / MIDDLE / LAST with perfusion, source, dose and peak
      on, fp64 and fp32, as achieved bytes per second against the touches of the table in csrc/bioheat.hpp, alternating in
      the same run with the wave solvers' stage pass (``rk4_stage_kernel``, kind 0: 12 touches), which has the same access shape;
  (b) a whole thermal step (4 stiffness applies + 4 stage passes) against the fused linear step on the same mesh, interleaved.

    python tools/time_bioheat.py [--parts ab] [--log profiles/time_bioheat.log]

Times: HIP events around back-to-back launches (a); wall clock around synchronised ``advance`` / ``rk4`` calls (b)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)

N_DOFS = 217**3
# vector touches per dof with pr and s on (LAST: + cem43 read and written as doubles, tmax read and written)
TOUCHES = {"FIRST": (5 + 3, 0), "MIDDLE": (7 + 3, 0), "LAST": (6 + 2 + 2, 2)}  # (of the field type, of double)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_bioheat.log"))
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    with measure.Log("time_bioheat", a.log) as log:
        run(a, log)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, bh, lib = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "bioheat", "_lib"))
    log.header()

    if "a" in a.parts:
        log(f"(a) one stage launch over {N_DOFS} dofs: event pair around 200 launches after 100 untimed, median of {a.rounds} rounds, "
            "alternating with the RK4 stage vector pass of the wave solvers (kind 0, 12 touches)")
        for dt_np in (np.float64, np.float32):
            tdt, ts = lib.torch_dtype(dt_np), np.dtype(dt_np).itemsize
            vec = [torch.rand(N_DOFS, dtype=torch.float64, device="cuda").to(tdt) for _ in range(8)]
            cem = torch.zeros(N_DOFS, dtype=torch.float64, device="cuda")
            rk4 = getattr(lib.load(), f"fus_rk4_stage_{lib.suffix(tdt)}")
            stage = getattr(lib.load(), f"fus_bioheat_stage_{lib.suffix(tdt)}")
            minv, pr, s, b, T0, Tn, acc, tmax = (x.data_ptr() for x in vec)

            def rk4_pass():
                lib.check(rk4(1e-9, 1e-9, 0, *(x.data_ptr() for x in vec), N_DOFS, N_DOFS, lib.stream_ptr()), "fus_rk4_stage")

            def bioheat_pass(kind):
                lib.check(stage(1e-9, 1e-9, kind, 1.0, 37.0, 1e-9, minv, pr, s, b, T0, Tn, acc, cem.data_ptr(), tmax, 0, N_DOFS, N_DOFS,
                                lib.stream_ptr()), "fus_bioheat_stage")

            cases = [("rk4 stage pass", 12 * N_DOFS * ts, rk4_pass)]
            for kind, name in enumerate(("FIRST", "MIDDLE", "LAST")):
                nt, nd = TOUCHES[name]
                cases.append((f"bioheat {name}", N_DOFS * (nt * ts + nd * 8), lambda kind=kind: bioheat_pass(kind)))
            res = measure.interleave({name: one for name, _, one in cases}, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
            ref = None
            for name, nb, _ in cases:
                st = measure.stats(res[name])
                bw = nb / (st.median * 1e-3) / 1e12
                ref = bw if ref is None else ref
                log(f"  {np.dtype(dt_np).name} {name:16s} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f})  model {nb / 1e6:7.1f} MB"
                    f"  {bw:.2f} TB/s  = {bw / ref:.3f} x the rk4 stage pass")
            del vec, cem, cases
            torch.cuda.empty_cache()

    if "b" in a.parts:
        K = 20
        log(f"(b) whole steps (P=4, 54^3 perturbed cells, fp64, G formed in the kernel), {K} steps per round, interleaved: the thermal step "
            "(4 stiffness applies + 4 stage passes; perfusion, source, dose and peak on) against the fused linear step")
        mesh = boxmesh.BoxMesh(4, 54, length=0.12, perturb=0.16, seed=0)
        h = ls.time_step_parameters(mesh, 4, 1500.0, 0.5e6, 0.12)
        dt_w, _, _ = ls.snap_time_step(h, 4, 1500.0, 0.5e6, 0.12)
        wave = ls.LinearSpectral3D(mesh, np.float64, fused=True)
        wave.init()
        th = bh.BioheatSpectral3D(mesh, np.float64, perfusion_rate=0.01)
        th.set_heat_source(torch.rand(th.nlocal, dtype=torch.float64, device="cuda") * 1e5)
        dt_t = th.stable_time_step()
        log(f"  stable_time_step() = {dt_t:.4g} s (lambda_max {th.lambda_max:.4g} 1/s), wave dt = {dt_w:.4g} s")
        wave.rk4(0.0, 1.0, dt_w, max_steps=3)
        th.advance(0.0, 3 * dt_t, dt_t)
        tw, tt = 3 * dt_w, 3 * dt_t

        def wave_steps():
            nonlocal tw
            tw, _ = wave.rk4(tw, 1.0, dt_w, max_steps=K)

        def thermal_steps():
            nonlocal tt
            tt, _ = th.advance(tt, 1e9, dt_t, max_steps=K)

        res = measure.interleave({"linear rk4_step": wave_steps, "bioheat step": thermal_steps}, a.rounds, lambda fn: measure.host_time(fn, K))
        base = measure.stats(res["linear rk4_step"]).median
        for kind, v in res.items():
            med = measure.stats(v).median
            log(f"  {kind:16s} {med:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in v)})  -> {med / base:.3f} x the linear step")


if __name__ == "__main__":
    main()
