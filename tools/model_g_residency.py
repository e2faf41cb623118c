#!/usr/bin/env python3
"""CPU model (numpy only) of how much of ``G`` the second of two consecutive general-G planned stiffness applies finds in the memory-side
cache (256 MiB on MI355X), for the two sweep directions (csrc/stiffness.hpp: mirror_block; knob FUS_TUNE_PLAN_SWEEP).

    python tools/model_g_residency.py [--config 4:54] [--itemsize 8] [--group 32] [--cache-mib 256]

The model: ONE fully associative LRU cache of ``capacity`` bytes whose unit is a batch.  A batch's footprint is what its workgroup moves:
its cells' G (6 n^3 T per cell), their index data as the rows kernel reads it (2 n^2 per cell, a compact run table and the count word per
batch), the cell constants, and the 128-byte lines of its distinct dofs twice (x gathered, y updated; a line shared by two batches is
charged to both: the model does not know that the second finds it).  The batches are touched in launch order (the placement of
group_block; mirrored for a downward launch), first launch then second; a batch of the second launch HITS if the cache still holds it.
Nothing else is modelled: no replacement policy but LRU, no associativity, no allocation rule for atomics, no other stream.  Printed: the
G bytes hit in the second launch for upwards-upwards and upwards-downwards.  ``lru_hits`` is the model, ``footprint`` the input."""
import argparse
import collections
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import model_x_fetch  # noqa: E402

CACHE = 256 << 20


def lru_hits(g_bytes, other_bytes, first, second, capacity=CACHE):
    """G bytes of the launch ``second`` (batch ids in launch order) found in an LRU cache of ``capacity`` bytes that the launch ``first``
    has just gone through.  ``g_bytes`` / ``other_bytes``: per batch, what it moves of G and of everything else."""
    size = np.asarray(g_bytes, dtype=np.int64) + np.asarray(other_bytes, dtype=np.int64)
    held, used, hit = collections.OrderedDict(), 0, 0
    for launch, order in ((0, first), (1, second)):
        for b in (int(v) for v in order):
            if b in held:
                held.move_to_end(b)
                hit += int(g_bytes[b]) if launch else 0
                continue
            held[b] = None
            used += int(size[b])
            while used > capacity:
                old, _ = held.popitem(last=False)
                used -= int(size[old])
    return hit


def footprint(P, cells, itemsize=8, run_stride=64):
    """(G bytes, other bytes) per batch of the box mesh ``cells``^3 at degree P, and the mesh's numbers"""
    boxmesh = __import__("fusgpu_loader").submodule("boxmesh")
    mesh = boxmesh.BoxMesh(P, cells)
    n, epb = P + 1, model_x_fetch.cells_per_batch(P)
    nbatch = -(-mesh.ncells // epb)
    ncell_b = np.minimum(epb, mesh.ncells - epb * np.arange(nbatch, dtype=np.int64))
    _, lines = model_x_fetch.batch_sets(mesh.dofmap, epb, itemsize)
    nlines = np.bincount(lines >> 32, minlength=nbatch)
    g = ncell_b * 6 * n**3 * itemsize
    other = ncell_b * (2 * n * n + itemsize) + 8 * run_stride + 4 + 2 * model_x_fetch.LINE * nlines
    return g, other, {"ncells": mesh.ncells, "ndofs": mesh.ndofs, "nbatch": nbatch, "cells_per_batch": epb}


def model(P, cells, itemsize=8, group=32, capacity=CACHE):
    """{'up_up': G bytes hit, 'up_down': ..., 'g_bytes': all of G, 'launch_bytes': the modelled footprint of a launch, ...}"""
    g, other, info = footprint(P, cells, itemsize)
    up = model_x_fetch.group_block(np.arange(info["nbatch"]), info["nbatch"], group)
    down = info["nbatch"] - 1 - up
    return dict(info, g_bytes=int(g.sum()), launch_bytes=int((g + other).sum()), up_up=lru_hits(g, other, up, up, capacity),
                up_down=lru_hits(g, other, up, down, capacity))


def lines_of(r):
    return [f"model (tools/model_g_residency.py, LRU): a launch moves {r['launch_bytes'] / 1e6:.1f} MB in {r['nbatch']} batches, {r['g_bytes'] / 1e6:.1f} MB of it G",
            f"  upwards then upwards:   {r['up_up'] / 1e6:6.1f} MB of G hit in the second launch ({100 * r['up_up'] / r['g_bytes']:.1f} % of G, {100 * r['up_up'] / r['launch_bytes']:.1f} % of the launch)",
            f"  upwards then downwards: {r['up_down'] / 1e6:6.1f} MB of G hit in the second launch ({100 * r['up_down'] / r['g_bytes']:.1f} % of G, {100 * r['up_down'] / r['launch_bytes']:.1f} % of the launch)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="4:54", help="P:cells-per-direction")
    ap.add_argument("--itemsize", type=int, default=8, choices=[4, 8])
    ap.add_argument("--group", type=int, default=32, help="g of the batch placement (0: natural order)")
    ap.add_argument("--cache-mib", type=int, default=256)
    a = ap.parse_args()
    P, N = (int(v) for v in a.config.split(":"))
    print(f"P={P} {N}^3, {a.itemsize}-byte scalars, g = {a.group}, cache {a.cache_mib} MiB")
    print("\n".join(lines_of(model(P, N, a.itemsize, a.group, a.cache_mib << 20))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
