#!/usr/bin/env python3
"""Point sensors on one MI355X (csrc/probe.hpp):

  (a) one sensor launch (``probe_eval_kernel<T, P>``) at 34 081 points -- the reference piston demo's 141 x 241 grid, here on the
      mid-y plane -- every output on (series row, peaks, harmonics 1 and 2), fp64 and fp32, P = 4 on config 3's 54^3 cells and
      P = 6 on 36^3 cells;
  (b) config-3 linear steps (P = 4, 54^3 perturbed cells, fp64, fused) without and with those sensors, interleaved;
  (c) the bowl demo's last-period window per step (Westervelt, fused, P = 4, 54^3 bowl-warped cells): the loop the demo runs without
      sensors -- ``rk4(max_steps=1)`` + ``u_sol()`` (a full-field copy to the host) per step -- against ONE ``rk4`` call recording
      every step on the device, and a plain ``rk4`` without either.

    python tools/time_sensors.py [--parts abc] [--log profiles/time_sensors.log]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_sensors.py --parts a     # the kernel by name

Times: HIP events around back-to-back launches / steps (the steps' times include every launch of ``rk4``)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)


def plane_points(L, nx=141, nz=241):
    x, z = np.linspace(0.0, L, nx), np.linspace(0.0, L, nz)
    X, Z = np.meshgrid(x, z, indexing="ij")
    return np.stack([X.reshape(-1), np.full(X.size, 0.5 * L), Z.reshape(-1)], axis=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_sensors.log"))
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args(argv)
    with measure.Log("time_sensors", a.log) as log:
        run(a, log)


def step_lines(log, res, width, what):
    base = measure.stats(next(iter(res.values()))).median
    for kind, v in res.items():
        med = measure.stats(v).median
        log(f"  {kind:{width}s} {med:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in v)})  -> {med / base:.4f} x {what}")
    for line in measure.verdict_lines(res, to_us=1e3):
        log(line)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, nls, sens = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "nonlinear_solver", "sensors"))
    log.header()
    L = 0.12
    pts = plane_points(L)

    if "a" in a.parts:
        log("(a) one sensor launch, 34081 points, series + peaks + harmonics 1, 2 (event pair around 200 launches, median of rounds)")
        for P, cells in ((4, 54), (6, 36)):
            t0 = time.perf_counter()
            mesh = boxmesh.BoxMesh(P, cells, length=L, perturb=0.16, seed=0)
            t_mesh = time.perf_counter() - t0
            for dt_np in (np.float64, np.float32):
                t0 = time.perf_counter()
                s = sens.PointSensors(mesh, pts, dt_np, capacity=1, peak=True, harmonics=(1, 2), frequency=0.5e6)
                t_setup = time.perf_counter() - t0
                u = torch.randn(mesh.ndofs, dtype=torch.float64, device="cuda").to(s.tdt)
                t = [0.0]

                def one():  # the series' single row is rewritten: every launch does all the work of a recording step
                    s.nrec = 0
                    t[0] += 1e-7
                    s.record(u, t[0])

                st = measure.stats(measure.interleave({"launch": one}, a.rounds, lambda fn: measure.event_time(fn, 200), warm=20)["launch"])
                nb = s.m * 3 * (P + 1) * s.tdt_np.itemsize + s._rows.numel() * 4 + s._rows.numel() * s.tdt_np.itemsize
                log(f"  P={P} {cells}^3 {np.dtype(dt_np).name}: {s.m} points in {s._rows.shape[0]} cells, "
                    f"{st.median * 1e3:.1f} us per launch (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f}); "
                    f"distinct input ~{nb / 1e6:.2f} MB; host set-up {t_setup:.2f} s (mesh {t_mesh:.1f} s)")
                del s, u
            del mesh
            torch.cuda.empty_cache()

    if "b" in a.parts:
        K = 20
        log(f"(b) config-3 linear step (P=4, 54^3 perturbed, fp64, fused): rk4 over {K} steps, without / with sensors, interleaved")
        mesh = boxmesh.BoxMesh(4, 54, length=L, perturb=0.16, seed=0)
        h = ls.time_step_parameters(mesh, 4, 1500.0, 0.5e6, L)
        dt, tf, _ = ls.snap_time_step(h, 4, 1500.0, 0.5e6, L)
        solver = ls.LinearSpectral3D(mesh, np.float64)
        solver.init()
        s = sens.PointSensors(mesh, pts, np.float64, capacity=K, peak=True, harmonics=(1, 2), frequency=0.5e6)
        solver.rk4(0.0, tf, dt, max_steps=3)
        t = 3 * dt

        def steps(sensors):
            def go():
                nonlocal t
                t, _ = solver.rk4(t, tf * 100, dt, max_steps=K, sensors=sensors)

            return s.reset, go

        step_lines(log, measure.interleave({"plain": steps(None), "sensors": steps(s)}, a.rounds, lambda fn: measure.host_time(fn, K)), 7, "plain")
        del solver, s
        torch.cuda.empty_cache()

    if "c" in a.parts:
        W = 30
        log(f"(c) bowl demo's last-period window (Westervelt, fused, P=4, 54^3 bowl-warped, fp64): {W} steps per variant, the first "
            "three interleaved, the host loop after them")
        Nc = 54

        def bowl(xg):
            out = xg.copy()
            yy, zz = xg[:, 1] / L - 0.5, xg[:, 2] / L - 0.5
            out[:, 0] = xg[:, 0] + 0.15 * (L / Nc) * 4 * (yy * yy + zz * zz) * (1.0 - xg[:, 0] / L)
            return out

        mesh = boxmesh.BoxMesh(4, Nc, length=L, warp=bowl)
        h = ls.time_step_parameters(mesh, 4, 1480.0, 1.1e6, L)
        dt = 0.40 * h / (1480.0 * 16)
        spp = int((1 / 1.1e6) / dt) + 1
        dt = (1 / 1.1e6) / spp
        solver = nls.WesterveltSpectral3D(mesh, np.float64, fused=True)
        solver.init()
        lex = mesh.global_lexicographic_ids()[: mesh.nlocal]
        gd = mesh.global_dof_dims
        on_plane = np.nonzero((lex % gd[2]) == gd[2] // 2)[0]
        s = sens.PointSensors(mesh, pts, np.float64, capacity=W, peak=True, harmonics=(1, 2), frequency=1.1e6)
        s0 = sens.PointSensors(mesh, pts, np.float64, capacity=W, peak=True)  # no harmonics: no per-step coefficient copy
        solver.rk4(0.0, 1.0, dt, max_steps=3)
        t = 3 * dt

        def between():  # untimed steps between the variants
            nonlocal t
            s.reset()
            s0.reset()
            t, _ = solver.rk4(t, 1.0, dt, max_steps=5)

        def steps(sensors):
            def go():
                nonlocal t
                t, _ = solver.rk4(t, 1.0, dt, max_steps=W, sensors=sensors)

            return between, go

        def host_loop():  # what demo_nonlinear_bowl.py does per step of its window without --sensor-plane
            nonlocal t
            for _ in range(W):
                t, _ = solver.rk4(t, 1.0, dt, max_steps=1)
                _ = solver.u_sol()[on_plane]

        def timer(fn):
            return measure.host_time(fn, W)

        res = measure.interleave({"plain": steps(None), "sensors": steps(s), "sensors, no harmonics": steps(s0)}, a.rounds, timer)
        # the host loop leaves the device idle most of the time (its clocks drop): it runs in a block of its own after the others
        res.update(measure.interleave({"host loop": (between, host_loop)}, 2, timer))
        step_lines(log, res, 21, "plain")
        log(f"  (field: {mesh.nlocal * 8 / 1e6:.1f} MB per u_sol() copy; {s.m} sensor points; steps per period {spp})")


if __name__ == "__main__":
    main()
