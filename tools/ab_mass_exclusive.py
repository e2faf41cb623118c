#!/usr/bin/env python3
"""Cell mass apply with and without exclusive-dof marks in the batch plan (csrc/plan.hpp, fus_plan_mark_exclusive), ~10 M
dofs per degree, K back-to-back launches between one HIP-event pair, alternating rounds.  Prints ms, TB/s of the
algorithmic bytes and the fraction of the plan's (batch, dof) sums that are finished without an atomic."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--degrees", default="4,2,3,5,6")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    import torch

    import fusgpu_loader
    import measure

    ops = fusgpu_loader.submodule("operators")
    lib = fusgpu_loader.submodule("_lib").load()
    for P in (int(v) for v in a.degrees.split(",")):
        n = P + 1
        pb = measure.device_problem(P, max(2, round((10.2e6) ** (1 / 3) / P)), np.float64, detJ=True)
        mesh, dm = pb.mesh, pb.dm
        opsd = {"atomics only": ops.mass_operator(n**3, np.float64, atomic=True), "exclusive marks": ops.mass_operator(n**3, np.float64, exclusive=True, atomic=True)}
        arms = {k: (lambda op=op: op(pb.x, pb.cc, pb.y, pb.detJ, dm)) for k, op in opsd.items()}
        err = measure.arms_agree(arms, pb.y)
        assert err < 1e-13, err
        res = measure.interleave(arms, a.rounds, lambda fn: measure.event_time(fn, a.reps, warm=1))
        ws, epb = ops._PLANS.get(dm, exclusive_ndofs=mesh.ndofs)
        nbatch = (mesh.ncells + epb - 1) // epb
        nbytes = int(lib.fus_plan_bytes(n**3, epb, mesh.ncells))
        words = (epb * n**3 + 31) // 32
        ex = ws[nbytes - ((nbatch * words * 4 + 255) // 256 * 256):][: nbatch * words * 4].view(torch.int32).cpu().numpy().view(np.uint32)
        marked = int(np.unpackbits(ex.view(np.uint8)).sum())
        nu = int((ws[256:256 + 4 * nbatch].view(torch.int32).cpu().numpy() & 0xFFFF).sum())
        bpc = n**3 * 8 + 4 * n**3 + 3 * 8 * P**3 + 8
        line = f"P={P} {mesh.ncells} cells {mesh.ndofs} dofs, {epb} cells/batch, {nu / nbatch:.0f} distinct dofs/batch, {100.0 * marked / nu:.1f} % exclusive:"
        for k, v in res.items():
            ms = measure.stats(v).median
            line += f"  {k} {ms:.4f} ms = {mesh.ncells * bpc / ms / 1e9:.2f} TB/s ({100 * mesh.ncells * bpc / ms / 1e9 / 8:.1f} %)"
        print(line, flush=True)
        for line in measure.verdict_lines(res, to_us=1e3):
            print(line, flush=True)
        del pb, dm, arms, opsd


if __name__ == "__main__":
    main()
