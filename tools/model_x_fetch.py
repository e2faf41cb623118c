#!/usr/bin/env python3
"""CPU model (numpy only) of how many bytes of ``x`` the general-G planned stiffness apply fetches into the XCDs' L2s per launch, for a
placement of the batches on the XCDs (csrc/stiffness.hpp: group_block).

    python tools/model_x_fetch.py [--config 4:54] [--groups 1,4,8,16,32,64,128] [--window 48] [--itemsize 8]

The model: a batch is ``cells_per_batch`` consecutive cells of the box mesh; it touches the 128-byte lines that hold its distinct dofs.
Workgroup ``bid`` runs on XCD ``bid % 8`` (a label: which workgroups share an L2), the workgroups of an XCD in the order of their ids.
A line is FETCHED by a batch unless the same XCD touched it within its last W batches.  Nothing else is modelled: no L2 capacity beyond the
window, no Infinity Cache, no other stream.  Printed: distinct dofs per cell, touches per dof, lines touched per 16 dofs touched, and per
placement the MB fetched per launch; ``chunks`` is FUS_TUNE_XCD_REMAP = 1 (one contiguous eighth of the batches per XCD), ``floor`` is x
read once."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

LINE = 128


def group_block(bid, nblocks, g):
    """csrc/stiffness.hpp group_block for an array of workgroup ids: g consecutive batches per XCD label, g a power of two (0, 1: natural)"""
    bid = np.asarray(bid, dtype=np.int64)
    if g < 2:
        return bid.copy()
    s = int(g).bit_length() - 1
    assert g == 1 << s, "group size: a power of two"
    full = nblocks & ~((8 << s) - 1)
    m, k = bid >> 3, bid & 7
    grouped = ((m >> s) << (3 + s)) + (k << s) + (m & (g - 1))
    return np.where(bid >= full, bid, grouped)


def chunk_block(bid, nblocks):
    """csrc/stiffness.hpp remap_block with the remap on: XCD label k walks one contiguous eighth of the batches"""
    bid = np.asarray(bid, dtype=np.int64)
    per, rem = nblocks >> 3, nblocks & 7
    xcd, idx = bid & 7, bid >> 3
    return xcd * per + np.minimum(xcd, rem) + idx


def cells_per_batch(P):
    return max(256 // ((P + 1) ** 2), 1)  # csrc/plan.hpp cells_per_batch


def batch_sets(dofmap, epb, itemsize):
    """(batch, dof) and (batch, line) pairs, each distinct, as two int64 arrays per kind"""
    ncell = dofmap.shape[0]
    batch = (np.arange(ncell, dtype=np.int64) // epb)[:, None]
    dofs = np.unique((batch << 32) | dofmap.astype(np.int64))
    lines = np.unique((batch << 32) | (dofmap.astype(np.int64) * itemsize // LINE))
    return dofs, lines


def fetched_lines(lines, nbatch, batch_of_block, window):
    """lines fetched per launch under the placement ``batch_of_block`` (workgroup id -> batch)"""
    bid = np.empty(nbatch, dtype=np.int64)
    bid[batch_of_block] = np.arange(nbatch)
    b, line = lines >> 32, lines & 0xFFFFFFFF
    xcd, seq = bid[b] & 7, bid[b] >> 3
    o = np.lexsort((seq, line, xcd))
    xcd, line, seq = xcd[o], line[o], seq[o]
    same = (xcd[1:] == xcd[:-1]) & (line[1:] == line[:-1])
    hit = same & (seq[1:] - seq[:-1] <= window)
    return int(line.size - hit.sum())


def model(P, cells, groups, window=48, itemsize=8):
    boxmesh = __import__("fusgpu_loader").submodule("boxmesh")
    mesh = boxmesh.BoxMesh(P, cells)
    epb = cells_per_batch(P)
    nbatch = -(-mesh.ncells // epb)
    dofs, lines = batch_sets(mesh.dofmap, epb, itemsize)
    out = {"ncells": mesh.ncells, "ndofs": mesh.ndofs, "nbatch": nbatch, "cells_per_batch": epb,
           "distinct_dofs_per_cell": dofs.size / mesh.ncells, "touches_per_dof": dofs.size / mesh.ndofs,
           "lines_per_16_dofs": lines.size * (LINE // itemsize) / dofs.size, "floor_mb": mesh.ndofs * itemsize / 1e6, "mb": {}}
    ids = np.arange(nbatch)
    for g in groups:
        out["mb"][g] = fetched_lines(lines, nbatch, group_block(ids, nbatch, g), window) * LINE / 1e6
    out["mb"]["chunks"] = fetched_lines(lines, nbatch, chunk_block(ids, nbatch), window) * LINE / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="4:54", help="P:cells-per-direction")
    ap.add_argument("--groups", default="1,4,8,16,32,64,128")
    ap.add_argument("--window", type=int, default=48, help="W: batches an XCD keeps a line for")
    ap.add_argument("--itemsize", type=int, default=8, choices=[4, 8])
    a = ap.parse_args()
    P, N = (int(v) for v in a.config.split(":"))
    r = model(P, N, [int(g) for g in a.groups.split(",")], a.window, a.itemsize)
    print(f"P={P} {N}^3: {r['ncells']} cells, {r['ndofs']} dofs, {r['nbatch']} batches of {r['cells_per_batch']} cells, W = {a.window}")
    print(f"  distinct dofs per cell {r['distinct_dofs_per_cell']:.2f}, touches per dof {r['touches_per_dof']:.3f}, "
          f"lines per {LINE // a.itemsize} dofs touched {r['lines_per_16_dofs']:.3f}")
    for g, mb in r["mb"].items():
        print(f"  g = {g!s:>6}: x fetch {mb:7.1f} MB per launch")
    print(f"  floor (x once): {r['floor_mb']:.1f} MB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
