"""
Point sensors: the field at a fixed set of physical points, evaluated on the device after every time step and recorded or
accumulated there (csrc/probe.hpp, ``fus_probe_eval_*``).

The reference keeps its output on the host: per step of its collection window it copies the whole field back and calls
dolfinx's ``Function.eval`` at the points ``compute_eval_params`` found once (cuda/utils.py:117-154,
cuda/demo_linear_piston.py, cuda/demo_nonlinear_bowl.py:662-680: ``u_n_.eval(x_eval, cell_eval)``).  Here the points are
located once on the host (``point_evaluation.CellLocator`` + its Newton inversion, the same arithmetic as
``eval_function``), their 1-D Lagrange rows are tabulated once, and each step costs one small launch inside ``rk4``
(which steps, and their harmonic factors on the device: ``recording.py``, shared with ``field_monitor.FieldMonitor``):

    s = PointSensors(mesh, points, np.float64, capacity=steps_per_period, peak=True, harmonics=(1, 2), frequency=f0)
    solver.rk4(t0, tf, dt, sensors=s, record_from=tf - period)
    s.series(), s.peak(), s.harmonic_amplitude(1)

Columns of every output follow ``point_ids`` (indices into the caller's point list, in device order: sorted by cell).
A partitioned run keeps, on every rank, every point that lies in one of its cells (as the reference's ranks do);
``merge`` / ``gather`` combine the ranks' columns into one array over the global list, the lowest rank taking a point
that several hold.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .gll import gll_points_weights
from .point_evaluation import CellLocator, _invert, _lagrange_1d
from .recording import SeriesRecorder, harmonic_coefficients  # noqa: F401  (harmonic_coefficients: re-exported)


@dataclass
class SensorSetup:
    """Host side of a sensor set: what is uploaded once."""

    point_ids: np.ndarray  # int64 [m]  indices into the caller's list, device order (sorted by cell)
    points: np.ndarray  # float64 [m, 3]
    cells: np.ndarray  # int64 [m]  the mesh cell of each point
    cell_index: np.ndarray  # int32 [m]  row of ``rows`` of each point
    rows: np.ndarray  # int32 [k, n^3]  dofmap rows of the k distinct cells, tensor-product local order
    weights: np.ndarray  # float64 [m, 3, n]  Lx, Ly, Lz of each point


def _as_points(points):
    """[m, 3] float64 from [m, 3] or the reference's 3 x m layout (cuda/utils.py:117)."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 1 and pts.size == 3:
        pts = pts[None, :]
    if pts.ndim != 2 or 3 not in pts.shape:
        raise ValueError(f"points: [m, 3] or 3 x m, got shape {pts.shape}")
    return np.ascontiguousarray(pts if pts.shape[1] == 3 else pts.T)


def sensor_setup(mesh, points, locator=None) -> SensorSetup:
    """Locate ``points`` in ``mesh`` (``P``, ``dofmap``, ``x_dofs``, ``x_g``) and tabulate their weights.  Points outside
    this rank's cells are dropped (``compute_eval_params``); the rest are sorted by cell."""
    pts = _as_points(points)
    P, n = int(mesh.P), int(mesh.P) + 1
    loc = locator if locator is not None else CellLocator(mesh.x_dofs, mesh.x_g)
    cell, _ = loc.locate(pts) if pts.shape[0] else (np.zeros(0, np.int64), None)
    ids = np.nonzero(cell >= 0)[0]
    ids = ids[np.argsort(cell[ids], kind="stable")]
    cells = cell[ids].astype(np.int64)
    p = pts[ids]
    w = np.zeros((ids.size, 3, n))
    if ids.size:
        # the reference coordinates exactly as eval_function forms them: Newton from the centre of the given cell
        xi, ok = _invert(np.asarray(mesh.x_g, dtype=np.float64)[np.asarray(mesh.x_dofs)[cells]], p)
        if not ok.all():
            raise ValueError("a located point could not be mapped into its cell")
        xi = np.clip(xi, 0.0, 1.0)
        nodes, _ = gll_points_weights(P)
        for a in range(3):
            w[:, a, :] = _lagrange_1d(nodes, xi[:, a])
    uniq, cell_index = np.unique(cells, return_inverse=True)
    rows = np.ascontiguousarray(np.asarray(mesh.dofmap)[uniq].astype(np.int32)).reshape(uniq.size, n**3)
    return SensorSetup(ids.astype(np.int64), p, cells, cell_index.astype(np.int32).reshape(-1), rows, w)


def merge(per_rank, npoints=None):
    """``per_rank``: ``[(point_ids, values), ...]`` in rank order, ``values`` with the points on the LAST axis.  Returns
    ``values`` over the global point list (``npoints`` columns, default: the largest id + 1); a point held by several
    ranks takes the lowest rank's value, a point held by none is NaN."""
    per_rank = [(np.asarray(i, dtype=np.int64), np.asarray(v)) for i, v in per_rank]
    if npoints is None:
        npoints = 1 + max((int(i.max()) for i, _ in per_rank if i.size), default=-1)
    lead = next((v.shape[:-1] for _, v in per_rank), ())
    out = np.full(lead + (int(npoints),), np.nan)
    for ids, vals in reversed(per_rank):  # the lowest rank writes last
        if vals.shape[:-1] != lead or vals.shape[-1] != ids.size:
            raise ValueError(f"merge: values of shape {vals.shape} for {ids.size} points (leading shape {lead} expected)")
        out[..., ids] = vals
    return out


class PointSensors(SeriesRecorder):
    """A fixed set of points of ``mesh``, evaluated on the device (``fus_probe_eval_*``).

    ``capacity``: rows of the time series (``record`` writes one per call; 0 = no series); ``peak``: running max / min;
    ``harmonics``: the multiples ``k`` of ``frequency`` whose complex amplitudes are accumulated."""

    def __init__(self, mesh, points, float_type=np.float64, capacity=0, peak=False, harmonics=(), frequency=None, locator=None):
        import torch

        self.P = int(mesh.P)
        self.npoints = int(_as_points(points).shape[0])
        self.setup = sensor_setup(mesh, points, locator)
        self.point_ids, self.points = self.setup.point_ids, self.setup.points
        self.m = m = self.point_ids.size
        super().__init__(float_type, mesh.ndofs, m, capacity, harmonics, frequency)
        if self.setup.rows.size and int(self.setup.rows.max()) >= self.ndofs:
            raise ValueError("dofmap row outside the local vector")
        dev = self.dev
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self._cells = td(self.setup.cell_index)
        self._rows = td(self.setup.rows)
        self._w = td(self.setup.weights.astype(self.tdt_np))
        self._pmax = torch.empty(m, dtype=torch.float64, device=dev) if peak else None
        self._pmin = torch.empty(m, dtype=torch.float64, device=dev) if peak else None
        self._fn = getattr(self._lib.load(), f"fus_probe_eval_{self._lib.suffix(self.tdt)}")
        self.reset()

    # -- device --------------------------------------------------------------------------------------------------------
    def _reset_more(self):
        if self._pmax is not None:
            self._pmax.fill_(-np.inf)
            self._pmin.fill_(np.inf)

    def _launch(self, u, rec, capacity, slot, pmax=None, pmin=None, hre=None, him=None, coef=None, H=0):
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._lib.check(
            self._fn(ptr(u), ptr(self._cells), self.m, ptr(self._rows), int(self._rows.shape[0]), ptr(self._w), self.P,
                     ptr(rec), int(capacity), int(slot), ptr(pmax), ptr(pmin), ptr(hre), ptr(him), ptr(coef), int(H),
                     self._lib.stream_ptr()),
            "fus_probe_eval",
        )

    def evaluate(self, u):
        """The field ``u`` (device, owned + ghosts, ghosts current) at the points: a device tensor [m] (columns of
        ``point_ids``) -- the device counterpart of ``point_evaluation.eval_function``."""
        import torch

        self._check_field(u)
        out = torch.empty((1, self.m), dtype=self.tdt, device=self.dev)
        self._launch(u, out, 1, 0)
        return out[0]

    def record(self, u, t):
        """One launch: row ``nrec`` of the series, the peaks and the harmonic terms of the field ``u`` at time ``t``."""
        self._check_record(u)
        coef, H = self.factors.row(t), len(self.harmonics)
        self._launch(u, self._rec, self.capacity, self.nrec, self._pmax, self._pmin, self._hre, self._him, coef, H)
        self._recorded()

    # -- host accessors ------------------------------------------------------------------------------------------------
    def series(self):
        """The recorded rows, ``[nrec, m]`` on the host."""
        if self._rec is None:
            return np.zeros((0, self.m), dtype=self.tdt_np)
        return self._rec[: self.nrec].cpu().numpy()

    def peak(self):
        """``(max, min)`` over the records, ``[m]`` each (fp64)."""
        if self._pmax is None:
            raise ValueError("this sensor set keeps no peaks (peak=False)")
        return self._pmax.cpu().numpy(), self._pmin.cpu().numpy()

    def harmonic_amplitude(self, k):
        """``(2 / N) |sum p e^{-i k w t}|`` over the N records: the amplitude of the k-th harmonic, exact for a periodic
        field sampled at N equal steps over one period (the solvers' ``dt = period / steps_per_period``)."""
        h = self.factors.index(k)
        if self.nacc == 0:
            return np.zeros(self.m)
        re, im = self._hre[h].cpu().numpy(), self._him[h].cpu().numpy()
        return 2.0 / self.nacc * np.hypot(re, im)

    def gather(self, comm, values=None):
        """``values`` (default: ``series()``; points on the last axis) of every rank merged over the global point list
        through the communicator's bootstrap (``scatterer.gather_arrays``).  Ranks driven from one process have none: use
        ``merge``."""
        from .scatterer import comm_size, gather_arrays

        values = self.series() if values is None else np.asarray(values)
        if comm_size(comm) == 1:
            return merge([(self.point_ids, values)], self.npoints)
        every = gather_arrays(comm, {"ids": self.point_ids, "values": values}, "gather", "sensors.merge")
        return merge([(z["ids"], z["values"]) for z in every], self.npoints)
