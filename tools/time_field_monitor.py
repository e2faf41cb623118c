#!/usr/bin/env python3
"""Full-field monitors on one MI355X (csrc/field_monitor.hpp), at config 3's size (P = 4, 54^3 cells: 217^3 =
10.2 M dofs -- config 5, P = 6 on 36^3 cells, has the same 217^3 dofs):

  (a) one monitor launch (``field_accumulate_kernel<T, H, W, NT>``) with peak / + both mean squares / + harmonics 1, 2, fp64 and
      fp32, as achieved bytes per second against the byte model n [T (1 + v) + 2 (2 T peak + 8 (nsq + 2 H))], alternating in the
      same run with the RK4 stage vector pass (``rk4_stage_kernel``, kind 0: 12 vector touches), which has the same access shape;
  (b) the fused linear step and the fused Westervelt step without and with a monitor (every output on), interleaved;
  (c) the bowl demo's last-period window per step: ONE ``rk4`` call with the monitor against the only full-field alternative
      without it -- ``rk4(max_steps=1)`` + ``u_sol()`` (a full-field copy to the host) per step -- and a plain ``rk4``;
  (p) a few launches of every variant of (a) and nothing else: the workload of a counter pass.

    python tools/time_field_monitor.py [--parts abc] [--log profiles/time_field_monitor.log]
    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE --output-format csv -d DIR -- python tools/time_field_monitor.py --parts p --log ""
    python tools/time_field_monitor.py --parts "" --pmc-dir DIR          # the kernel's HBM bytes of that pass against the model

Times: HIP events around back-to-back launches (a); wall clock around synchronised ``rk4`` calls (b, c)."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)

N_DOFS = 217**3
VARIANTS = (("peak", dict(peak=True)),
            ("peak + <u^2>, <v^2>", dict(peak=True, mean_square=("u", "v"))),
            ("peak + <u^2>, <v^2> + H1, H2", dict(peak=True, mean_square=("u", "v"), harmonics=(1, 2), frequency=0.5e6)))


def model_bytes(n, tsize, peak, nsq, H, v):
    return n * (tsize * (1 + v) + 2 * (2 * tsize * peak + 8 * (nsq + 2 * H)))


def variant_bytes(n, tsize, kw):
    nsq = len(kw.get("mean_square", ()))
    return model_bytes(n, tsize, int(bool(kw.get("peak"))), nsq, len(kw.get("harmonics", ())), int("v" in kw.get("mean_square", ())))


def pmc_summary(pmc_dir, log):
    """HBM bytes per launch of the monitor kernels in a ``rocprofv3 --pmc FETCH_SIZE WRITE_SIZE`` pass of part (p): gfx950's FETCH_SIZE
    counts half of wide reads (docs/history.md), so bytes = (2 FETCH_SIZE + WRITE_SIZE) x 1024."""
    files = glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        log(f"(p) no counter_collection.csv under {pmc_dir}")
        return
    per = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            if "field_accumulate_kernel" in r["Kernel_Name"]:
                per.setdefault(r["Kernel_Name"].split("(")[0], {}).setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    log(f"(p) HBM bytes per launch from {os.path.basename(os.path.normpath(pmc_dir))}: (2 FETCH_SIZE + WRITE_SIZE) x 1024, n = {N_DOFS}")
    for k, c in sorted(per.items()):
        fetch, write = (measure.stats(c.get(counter, [np.nan])).median for counter in ("FETCH_SIZE", "WRITE_SIZE"))
        log(f"  {k.replace('void fus::', '')}: {len(c.get('FETCH_SIZE', []))} launches, read {2 * fetch * 1024 / 1e6:.1f} MB, "
            f"written {write * 1024 / 1e6:.1f} MB, total {(2 * fetch + write) * 1024 / 1e6:.1f} MB")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_field_monitor.log"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pmc-dir", default=None)
    a = ap.parse_args(argv)
    with measure.Log("time_field_monitor", a.log) as log:
        if a.pmc_dir:
            pmc_summary(a.pmc_dir, log)
        if a.parts:
            run(a, log)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, nls, fm, lib, sens = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "nonlinear_solver", "field_monitor",
                                                                             "_lib", "sensors"))
    log.header()
    L = 0.12

    def launches(dt_np):
        """[(name, model bytes, callable)] of the monitor variants on random fields of N_DOFS values."""
        tdt = lib.torch_dtype(dt_np)
        u = torch.randn(N_DOFS, dtype=torch.float64, device="cuda").to(tdt)
        v = torch.randn(N_DOFS, dtype=torch.float64, device="cuda").to(tdt)
        out = []
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        for name, kw in VARIANTS:
            m = fm.FieldMonitor(N_DOFS, dt_np, **kw)
            H = len(m.harmonics)
            coef = torch.from_numpy(sens.harmonic_coefficients(m.harmonics, m.omega, 1e-7)).cuda() if H else None
            m.record(u, v, 1e-7)  # the init record; the timed launches read and write every accumulator

            def one(m=m, H=H, coef=coef):  # the launch of FieldMonitor.record with this step's factors already on the device
                lib.check(m._fn(u.data_ptr(), ptr(v) if m._vsq is not None else None, N_DOFS, ptr(m._pmax), ptr(m._pmin), ptr(m._usq),
                                ptr(m._vsq), ptr(m._hre), ptr(m._him), m.npad, ptr(coef), H, 0, lib.stream_ptr()), "fus_field_accumulate")

            out.append((name, variant_bytes(N_DOFS, np.dtype(dt_np).itemsize, kw), one))
        return out

    if "p" in a.parts:
        for dt_np in (np.float64, np.float32):
            for name, nb, one in launches(dt_np):
                for _ in range(5):
                    one()
                torch.cuda.synchronize()
                log(f"(p) {np.dtype(dt_np).name} {name}: model {nb / 1e6:.1f} MB per launch")

    if "a" in a.parts:
        log(f"(a) one monitor launch over {N_DOFS} dofs: event pair around 200 launches after 100 untimed, median of {a.rounds} rounds, "
            "alternating with the RK4 stage vector pass (kind 0, 12 touches)")
        for dt_np in (np.float64, np.float32):
            tdt, ts = lib.torch_dtype(dt_np), np.dtype(dt_np).itemsize
            vec = [torch.randn(N_DOFS, dtype=torch.float64, device="cuda").to(tdt) for _ in range(8)]
            stage = getattr(lib.load(), f"fus_rk4_stage_{lib.suffix(tdt)}")

            def stage_pass():  # MIDDLE: reads b minv ku u v u0 v0, writes u v un ku b
                lib.check(stage(1e-9, 1e-9, 0, *(x.data_ptr() for x in vec), N_DOFS, N_DOFS, lib.stream_ptr()), "fus_rk4_stage")

            cases = [("rk4 stage pass", 12 * N_DOFS * ts, stage_pass)] + launches(dt_np)
            res = measure.interleave({name: one for name, _, one in cases}, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
            ref = None
            for name, nb, _ in cases:
                st = measure.stats(res[name])
                bw = nb / (st.median * 1e-3) / 1e12
                ref = bw if ref is None else ref
                log(f"  {np.dtype(dt_np).name} {name:30s} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f})  model {nb / 1e6:7.1f} MB"
                    f"  {bw:.2f} TB/s  = {bw / ref:.3f} x the stage pass")
            del vec, cases
            torch.cuda.empty_cache()

    def step_rounds(solver, dt, monitor, K, rounds, t):
        def steps(m):
            def go():
                nonlocal t
                t, _ = solver.rk4(t, 1.0, dt, max_steps=K, monitor=m)

            return monitor.reset, go

        return measure.interleave({"plain": steps(None), "monitor": steps(monitor)}, rounds, lambda fn: measure.host_time(fn, K)), t

    if "b" in a.parts:
        K = 20
        log(f"(b) fused step (P=4, 54^3, fp64) over {K} steps without / with a monitor (peak, <u^2>, <v^2>, H1, H2), interleaved")
        for which in ("linear", "westervelt"):
            mesh = boxmesh.BoxMesh(4, 54, length=L, perturb=0.16, seed=0)
            c0, f0 = (1500.0, 0.5e6) if which == "linear" else (1480.0, 1.1e6)
            h = ls.time_step_parameters(mesh, 4, c0, f0, L)
            dt, _, _ = ls.snap_time_step(h, 4, c0, f0, L)
            solver = ls.LinearSpectral3D(mesh, np.float64, fused=True) if which == "linear" else nls.WesterveltSpectral3D(mesh, np.float64, fused=True)
            solver.init()
            m = fm.FieldMonitor(solver.nlocal, np.float64, peak=True, mean_square=("u", "v"), harmonics=(1, 2), frequency=f0)
            solver.rk4(0.0, 1.0, dt, max_steps=3)
            res, _ = step_rounds(solver, dt, m, K, a.rounds, 3 * dt)
            mp, mw = measure.stats(res["plain"]).median, measure.stats(res["monitor"]).median
            log(f"  {which:10s} plain   {mp:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in res['plain'])})")
            log(f"  {which:10s} monitor {mw:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in res['monitor'])})  -> {mw / mp:.4f} x, "
                f"+{(mw - mp) * 1e3:.0f} us")
            log(*measure.verdict_lines(res, to_us=1e3, indent=f"  {which:10s} "))
            del solver, m, mesh
            torch.cuda.empty_cache()

    if "c" in a.parts:
        W, Nc = 30, 54
        log(f"(c) bowl demo's last-period window (Westervelt, fused, P=4, 54^3 bowl-warped, fp64): {W} steps per variant, plain and monitor "
            "interleaved, the host loop after them")

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
        m = fm.FieldMonitor(solver.nlocal, np.float64, peak=True, mean_square=("u", "v"), harmonics=(1, 2), frequency=1.1e6)
        solver.rk4(0.0, 1.0, dt, max_steps=3)
        res, t = step_rounds(solver, dt, m, W, a.rounds, 3 * dt)

        def host_loop():  # what a caller without a monitor does per step of the window to see the whole field
            nonlocal t
            for _ in range(W):
                t, _ = solver.rk4(t, 1.0, dt, max_steps=1)
                _ = solver.u_sol()

        # the host loop leaves the device idle most of the time (its clocks drop): a block of its own, last
        res.update(measure.interleave({"host loop": host_loop}, 2, lambda fn: measure.host_time(fn, W)))
        med = {kind: measure.stats(v).median for kind, v in res.items()}
        for kind, v in res.items():
            log(f"  {kind:10s} {med[kind]:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in v)})  -> {med[kind] / med['plain']:.3f} x plain")
        for line in measure.verdict_lines(res, to_us=1e3):
            log(line)
        log(f"  host loop / monitor = {med['host loop'] / med['monitor']:.2f} x  "
            f"(field: {mesh.nlocal * 8 / 1e6:.1f} MB per u_sol() copy; steps per period {spp})")


if __name__ == "__main__":
    main()
