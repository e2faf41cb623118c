#!/usr/bin/env python3
"""Absorbing sponge layer on one MI355X (csrc/sponge.hpp), at config 3's size (P = 4, 54^3 perturbed cells: 217^3 =
10.2 M dofs), a layer of ``--cells`` cells (6) inside the four lateral faces:

  (a) the fused linear step without and with the layer, interleaved;
  (b) the layer's launch alone (``sponge_terms_kernel``), fp64 and fp32, as achieved bytes per second against the byte model
      n (4 + 5 sizeof(T)): the index, two coefficients, two gathered reads and one atomic add (a read and a write) per list entry.

    python tools/time_sponge.py [--parts ab] [--cells 6] [--log profiles/time_sponge.log]

Times: wall clock around synchronised ``rk4`` calls (a); HIP events around back-to-back launches (b)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import measure  # noqa: E402  (no torch at its module level)


def model_bytes(n, tsize):
    return n * (4 + 5 * tsize)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--cells", type=int, default=6, help="width of the layer in cells")
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--mesh-cells", type=int, default=54)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_sponge.log"))
    a = ap.parse_args(argv)
    with measure.Log("time_sponge", a.log) as log:
        run(a, log)


def run(a, log):
    import torch

    import fusgpu_loader

    torch.cuda.set_device(0)
    boxmesh, ls, sp, ops, lib = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "sponge", "operators", "_lib"))
    log.header()
    P, N, L, c0, f0 = a.degree, a.mesh_cells, 0.12, 1500.0, 0.5e6
    mesh = boxmesh.BoxMesh(P, N, length=L, perturb=0.16, seed=0)
    width = a.cells * L / N
    sigma = sp.box_profile((0.0, 0.0, 0.0), mesh.length, width, sp.LATERAL, c0)
    h = ls.time_step_parameters(mesh, P, c0, f0, L)
    dt, _, _ = ls.snap_time_step(h, P, c0, f0, L)
    layer = sp.SpongeLayer(sigma)
    idx, sig = layer.build(mesh)
    log(f"P = {P}, {N}^3 cells, {mesh.nlocal} dofs; layer of {a.cells} cells inside the lateral faces: {idx.size} dofs "
        f"({100 * idx.size / mesh.nlocal:.1f} %), sigma_max dt = {layer.sigma_max * dt:.3f}")

    if "a" in a.parts:
        K = a.steps
        log(f"(a) fused linear step (fp64) over {K} steps without / with the layer, interleaved, {a.rounds} rounds")
        solvers = {"plain": ls.LinearSpectral3D(mesh, np.float64, fused=True),
                   "sponge": ls.LinearSpectral3D(mesh, np.float64, fused=True, sponge=layer)}
        clock = {}
        for name, s in solvers.items():
            s.init()
            clock[name], _ = s.rk4(0.0, 1.0, dt, max_steps=3)

        def steps(name):
            def go():
                clock[name], _ = solvers[name].rk4(clock[name], 1.0, dt, max_steps=K)

            return go

        res = measure.interleave({name: steps(name) for name in solvers}, a.rounds, lambda fn: measure.host_time(fn, K))
        mp, mw = (measure.stats(res[k]).median for k in ("plain", "sponge"))
        for name in solvers:
            log(f"  {name:7s} {measure.stats(res[name]).median:.3f} ms/step  (rounds {', '.join(f'{x:.3f}' for x in res[name])})")
        log(f"  sponge / plain = {mw / mp:.4f} x, {(mw - mp) * 1e3:+.0f} us per step (4 launches)")
        for line in measure.verdict_lines(res, to_us=1e3):
            log(line)
        del solvers
        torch.cuda.empty_cache()

    if "b" in a.parts:
        log(f"(b) the layer's launch alone over {idx.size} list entries: event pair around 200 launches after 100 untimed, median of {a.rounds} rounds")
        for dt_np in (np.float64, np.float32):
            tdt, ts = lib.torch_dtype(dt_np), np.dtype(dt_np).itemsize
            y, u, v, m = (torch.rand(mesh.ndofs, dtype=torch.float64, device="cuda").to(tdt) for _ in range(4))
            bound = layer.bind(m, tdt, y.device, built=(idx, sig * 1e-9))  # small coefficients: y stays finite over thousands of launches
            res = measure.interleave({"sponge": lambda: ops.sponge_terms(y, u, v, bound)}, a.rounds, lambda fn: measure.event_time(fn, 200), warm=100)
            st = measure.stats(res["sponge"])
            nb = model_bytes(idx.size, ts)
            log(f"  {np.dtype(dt_np).name} {st.median * 1e3:7.1f} us (min {st.min * 1e3:.1f}, max {st.max * 1e3:.1f})  model {nb / 1e6:6.1f} MB"
                f"  {nb / (st.median * 1e-3) / 1e12:.2f} TB/s")
            del y, u, v, m, bound
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
