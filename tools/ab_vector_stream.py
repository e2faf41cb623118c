#!/usr/bin/env python3
"""FUS_TUNE_VECTOR_STREAM policies on one box: 0 cached, 3 non-temporal stores only, 1 non-temporal loads + stores (default) --
the fused RK4 step (general G), the cached-diagonal mass apply (3 vectors of 82 MB: fit the 256 MB Infinity Cache together) and
copy / axpy on 1 GiB operands."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODES = {"cached accesses": 0, "non-temporal stores only": 3, "non-temporal loads + stores (default)": 1}


def main(argv=None):
    argparse.ArgumentParser(description=__doc__).parse_args(argv)
    import torch

    import fusgpu_loader
    import measure

    lib_mod, ops, boxmesh, ls = (fusgpu_loader.submodule(m) for m in ("_lib", "operators", "boxmesh", "linear_solver"))
    torch.cuda.set_device(0)
    L = 0.12
    mesh = boxmesh.BoxMesh(4, 54, length=L)
    h = ls.time_step_parameters(mesh, 4, 1500.0, 0.5e6, L)
    dt, tf, _ = ls.snap_time_step(h, 4, 1500.0, 0.5e6, L)
    s = ls.LinearSpectral3D(mesh, np.float64, fused=True, affine=False)
    s.init()
    s.rk4(0.0, tf, dt, max_steps=3)
    n = mesh.ndofs
    w, x, y = (torch.randn(n, dtype=torch.float64, device="cuda") for _ in range(3))
    big, big2 = torch.ones((1 << 30) // 8, dtype=torch.float64, device="cuda"), torch.ones((1 << 30) // 8, dtype=torch.float64, device="cuda")
    fn_muladd = lib_mod.load().fus_muladd_f64
    parts = {"step": lambda: s.rk4(3 * dt, tf, dt, max_steps=40),
             "muladd": lambda: fn_muladd(w.data_ptr(), x.data_ptr(), y.data_ptr(), n, lib_mod.stream_ptr()),
             "copy": lambda: ops.copy(big, big2), "axpy": lambda: ops.axpy(big.numel())(0.5, big, big2)}

    # a round of a policy is four measurements, so the rounds are walked here: 40 solver steps on the wall clock (ms per step),
    # then the three kernels between events (us)
    res = {name: [] for name in MODES}
    for order in measure.round_schedule(MODES, 2):
        for name in order:
            lib_mod.set_tuning(lib_mod.TUNE_VECTOR_STREAM, MODES[name])
            res[name].append((measure.host_time(parts["step"], 40),)
                             + tuple(measure.event_time(parts[k], reps, warm=1) * 1e3 for k, reps in (("muladd", 50), ("copy", 10), ("axpy", 10))))
    lib_mod.set_tuning(lib_mod.TUNE_VECTOR_STREAM, 1)
    for rnd in range(2):
        for name, v in res.items():
            step, ma, cp, ax = v[rnd]
            print(f"round {rnd}: {name:32s} RK4 step {step:.3f} ms | muladd (3 x 82 MB) {ma:6.1f} us = {3 * 8 * n / ma / 1e6:.2f} TB/s | copy 1 GiB {2 * (1 << 30) / cp / 1e6:.2f} TB/s | "
                  f"axpy 1 GiB {3 * (1 << 30) / ax / 1e6:.2f} TB/s", flush=True)
    for line in measure.verdict_lines({name: [t[0] * 1e3 for t in v] for name, v in res.items()}, indent="RK4 step: "):
        print(line, flush=True)


if __name__ == "__main__":
    main()
