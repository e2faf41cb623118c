"""The order in which ``HaloApply.schedule()`` issues its work, pinned on the CPU with stand-ins (no GPU, no process group):
exchange begin / end, the yields, the cell sub-ranges and the boundary terms of the sequential and the split schedule, cell
split and row split; and what ``bootstrap_of`` / ``gather_floats`` make of communicators with and without a bootstrap."""

import types

import numpy as np
import pytest
import torch

from conftest import pkg
from halo_cpu import OracleHaloKernels


class _Closure:
    """A scatter closure that only records."""

    def __init__(self, log, tag):
        self.log, self.tag = log, tag

    def begin(self, vec):
        self.log.append(f"begin {self.tag}")
        return None

    def end(self, vec, work):
        self.log.append(f"end {self.tag}")


def _halo(overlap, lead_cells):
    scat = pkg("scatterer")
    comm = types.SimpleNamespace(rank=0, size=1)
    mesh = types.SimpleNamespace(nlocal=10, ncells=12, num_boundary_cells=2, dofmap=np.zeros((12, 27), dtype=np.int32))
    plan = ([[0, 1], [2], [0, 2], [0]], [[3, 4], [2], [0, 2], [0]])  # a rank that is its own neighbour
    return scat.HaloApply(mesh, None, comm, np.float64, overlap=overlap, kernels=OracleHaloKernels(), apply_fn=lambda *a: None,
                          plan=plan, lead_cells=lead_cells, schedule="split")


def _drive(halo, by_rows=False, facets=True):
    log = []
    vec = torch.zeros(14, dtype=torch.float64)
    if by_rows:
        percell, cell_fn = (), (lambda which: log.append(("rows", which)))
    else:
        percell, cell_fn = (torch.arange(12),), (lambda ids: log.append(("cells", ids.tolist())))
    terms = (lambda: log.append("facets")) if facets else None
    for what in halo.schedule(cell_fn, percell, [(_Closure(log, "f"), vec)], [(_Closure(log, "r"), vec)], terms, by_rows=by_rows):
        log.append(f"yield {what}")
    return log


def test_split_schedule_with_lead_slices():
    h = _halo(True, 2)
    assert (h.schedule_kind, h.lead_cells) == ("split", 2)
    assert h.ranges == {"boundary": (0, 2), "lead1": (2, 4), "interior1": (4, 7), "lead2": (7, 9), "interior2": (9, 12),
                        "interior": (2, 12)}
    assert _drive(h) == ["begin f", "yield forward", ("cells", [2, 3]), ("cells", [4, 5, 6]), "end f", ("cells", [0, 1]), "facets",
                         "begin r", "yield reverse", ("cells", [7, 8]), ("cells", [9, 10, 11]), "end r"]


def test_sequential_schedule():
    h = _halo(False, 2)
    assert (h.schedule_kind, h.lead_cells) == ("sequential", 0)
    assert _drive(h) == ["begin f", "yield forward", "end f", ("cells", [0, 1]), ("cells", [2, 3, 4, 5, 6]),
                         ("cells", [7, 8, 9, 10, 11]), "facets", "begin r", "yield reverse", "end r"]


def test_split_schedule_without_lead_slices():
    h = _halo(True, 0)
    assert (h.schedule_kind, h.lead_cells) == ("split", 0)
    assert _drive(h) == ["begin f", "yield forward", ("cells", [2, 3, 4, 5, 6]), "end f", ("cells", [0, 1]), "facets",
                         "begin r", "yield reverse", ("cells", [7, 8, 9, 10, 11]), "end r"]


def test_split_schedule_by_rows():
    """Set A where the first interior launch is, set B where the boundary cells are, nothing in the lead and second interior positions."""
    assert _drive(_halo(True, 2), by_rows=True, facets=False) == [
        "begin f", "yield forward", ("rows", 0), "end f", ("rows", 1), "begin r", "yield reverse", "end r"]


def test_sequential_schedule_by_rows():
    assert _drive(_halo(False, 2), by_rows=True) == [
        "begin f", "yield forward", "end f", ("rows", 1), ("rows", 0), "facets", "begin r", "yield reverse", "end r"]


def test_overlapped_row_split_refuses_boundary_terms():
    with pytest.raises(ValueError, match="boundary_terms"):
        _drive(_halo(True, 2), by_rows=True, facets=True)


class _Gathers:
    """A two-rank communicator stand-in whose all-gather returns this rank's payload and a second copy of it."""

    rank, size = 0, 2

    def allgather_bytes(self, payload):
        return [payload, payload]


def test_bootstrap_of_and_gather_floats():
    scat, comm = pkg("scatterer"), pkg("comm")
    assert scat.bootstrap_of is comm.bootstrap_of and scat.gather_floats is comm.gather_floats
    with_gather, without = _Gathers(), types.SimpleNamespace(rank=0, size=2)
    assert comm.bootstrap_of(with_gather) is with_gather
    assert comm.bootstrap_of(without) is None
    assert comm.bootstrap_of(None) is None
    got = comm.gather_floats(with_gather, [1.5, -2.0])
    assert got.dtype == np.float64 and np.array_equal(got, [[1.5, -2.0], [1.5, -2.0]])
    for c in (without, None):  # no process group is initialised here: the local row
        got = comm.gather_floats(c, [1.5, -2.0])
        assert got.dtype == np.float64 and np.array_equal(got, [[1.5, -2.0]])
