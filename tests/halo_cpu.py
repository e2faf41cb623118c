"""Test-only stand-ins injected into the product's scatterer / HaloApply so the
N > 1 host logic (partition, halo plan, exchange ordering) runs under gloo on
CPU tensors.  Backed by the ORACLE; never imported by the product."""

import numpy as np
import torch

from conftest import ref_field
from oracle import oracle_np, rk4_oracle


class OracleHaloKernels:
    def __init__(self, dtype=torch.float64):
        self.dtype = dtype

    def index_tensor(self, idx_np):
        return torch.from_numpy(np.ascontiguousarray(idx_np, dtype=np.int64))

    def buffer(self, n):
        return torch.zeros(int(n), dtype=self.dtype)

    def pack_fwd(self, in_, out, index):
        oracle_np.pack(in_.numpy(), out.numpy(), index.numpy())

    def unpack_fwd(self, in_, out, index, N):
        oracle_np.unpack_fwd(in_.numpy(), out.numpy()[N:], index.numpy())

    def pack_rev(self, in_, out, index, N):
        oracle_np.pack(in_.numpy()[N:], out.numpy(), index.numpy())

    def unpack_rev(self, in_, out, index):
        oracle_np.unpack_rev(in_.numpy(), out.numpy(), index.numpy())


def global_cell_constants(mesh, dtype=np.float64):
    """Rank-independent per-cell constants (function of the global cell index)."""
    ijk = mesh._cell_ijk + np.array([mesh.cell_range[a][0] for a in range(3)])[None, :]
    return (1.0 + 0.1 * ((ijk[:, 0] * 7 + ijk[:, 1] * 3 + ijk[:, 2]) % 5)).astype(dtype)


def stale_ghost_input(mesh):
    """The reference's test field on one rank's dofs, its ghost entries stale (-777) until a forward scatter refreshes them."""
    x = ref_field(mesh.dof_coordinates())
    x[mesh.nlocal:] = -777.0
    return x


def rank_inputs(mesh, dev, factor="G"):
    """One rank's operands of a partitioned fp64 apply as tensors on ``dev``: the stale-ghost input ``x``, a zero ``y``, the
    rank-independent cell constants ``cc``, the dofmap ``dm`` and the cells' geometry factor under its name, ``G`` (stiffness) or
    ``detJ`` (mass), from the oracle's host recipe (rk4_oracle.host_G / host_detJ; conftest.build_problem, which makes the serial
    side of these comparisons, keeps its own copy)."""
    geom = {"G": rk4_oracle.host_G, "detJ": rk4_oracle.host_detJ}[factor](mesh)
    to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return {"mesh": mesh, "x": to(stale_ghost_input(mesh)), "y": torch.zeros(mesh.ndofs, dtype=torch.float64, device=dev),
            "cc": to(global_cell_constants(mesh)), factor: to(geom), "dm": to(mesh.dofmap)}
