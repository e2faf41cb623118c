"""
Element receivers and time reversal: what each element of a transducer array RECEIVES, integrated over its face on the device after
every time step (csrc/element_receive.hpp, ``fus_element_receive_*``), and the array that fires the conjugate phases back.

A piezo element integrates pressure over its face: ``S_e(t) = int_{Gamma_e} u dS``.  ``ElementReceivers`` assigns the receiving facets
(default: the source-tagged set) to elements exactly as ``sources.SourceArray`` does -- the same ``element_of_facet`` gives the same
elements to transmit and to receive, and agrees across ranks -- sorts their facet-dof entries by element into one list with CSR
offsets, and each recorded step costs one small launch inside ``rk4`` (which steps, and their harmonic factors: ``recording.py``,
shared with ``sensors.PointSensors``).  The device holds INTEGRALS; the host divides by the element's area ``A_e = sum wgt`` at
harvest, after the partial integrals and partial areas of partitioned ranks are added (``merge`` / ``gather``).

Time reversal, the standard planning step of transcranial focusing: a virtual point source at the target, a receive run through the
heterogeneous medium, then the array fired with the conjugate phases.  The discrete problem is reciprocal (diagonal lumped mass,
symmetric K, diagonal absorbing term), so what element e receives from the point equals, up to a constant, what the point sees when
element e fires alone, and the conjugate phases put every element's contribution in phase at the target:

    rx = ElementReceivers(mesh, grid, np.float64, harmonics=(1,), frequency=f0)
    listen = LinearSpectral3D(mesh, speed_of_sound=c_cells, source_amplitude=0.0, point_source=PointSources(focus))
    listen.rk4(0.0, tf, dt, receivers=rx, record_from=tf - period)
    fire = LinearSpectral3D(mesh, speed_of_sound=c_cells, source=time_reversal(rx))
"""

from __future__ import annotations

import numpy as np

from .recording import SeriesRecorder
from .sources import SourceArray


def element_entries(ids, facet_dofmap, facet_detJ, n_elements):
    """The CSR layout of a receiving array on the host: ``(dof int32 [K], wgt [K], offsets int64 [E + 1])`` -- the facet-dof entries of
    the facets with ``ids[f] >= 0``, sorted by element (stable: facet order, then the facet's local order, within an element)."""
    ids = np.asarray(ids).reshape(-1)
    dm, dj = np.asarray(facet_dofmap), np.asarray(facet_detJ)
    if ids.size == 0:  # a rank without receiving facets: every element is empty here
        return np.zeros(0, np.int32), np.zeros(0, dj.dtype), np.zeros(int(n_elements) + 1, np.int64)
    dm, dj = dm.reshape(ids.size, -1), dj.reshape(ids.size, -1)
    if dm.shape != dj.shape:
        raise ValueError(f"facet dofmap {dm.shape} and facet detJ {dj.shape} differ in shape")
    e_of_entry = np.repeat(ids, dm.shape[1])
    act = np.nonzero(e_of_entry >= 0)[0]
    order = act[np.argsort(e_of_entry[act], kind="stable")]
    counts = np.bincount(e_of_entry[act], minlength=int(n_elements))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return np.ascontiguousarray(dm.reshape(-1)[order].astype(np.int32)), np.ascontiguousarray(dj.reshape(-1)[order]), offsets


def merge(per_rank):
    """``per_rank``: ``[(areas [E], integrals [..., E]), ...]``, one pair per rank -- the partial areas and the partial integrals (a
    series, or the complex harmonic sums) of each.  Both ADD over the ranks before the division: returns the area averages over the
    whole elements, NaN for an element without area on any rank."""
    per_rank = [(np.asarray(a, dtype=np.float64), np.asarray(v)) for a, v in per_rank]
    if not per_rank:
        raise ValueError("merge: no ranks")
    area = sum(a for a, _ in per_rank)
    total = sum(v for _, v in per_rank)
    if total.shape[-1:] != area.shape:
        raise ValueError(f"merge: integrals of shape {total.shape} for {area.size} elements")
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(area > 0, total / np.where(area > 0, area, 1.0), np.nan)


class ElementReceivers(SeriesRecorder):
    """The elements of a receiving array on ``mesh`` (see the module docstring).

    ``element_of_facet`` / ``n_elements``: as ``sources.SourceArray`` (the assignment IS ``SourceArray.assign``); ``facets``: the
    receiving ``(cell, local facet)`` rows (default: ``mesh.boundary_facets([source_tag])``); ``capacity``: rows of the time series
    (0 = none); ``harmonics``: the multiples ``k`` of ``frequency`` whose complex amplitudes are accumulated; ``detJ``: the scaled facet
    ``detJ`` of ``facets`` where the caller holds it already (a solver's ``detJ_f1``), else computed here on the device."""

    def __init__(self, mesh, element_of_facet, float_type=np.float64, capacity=0, harmonics=(), frequency=None, n_elements=None,
                 facets=None, detJ=None):
        import torch

        self.element_of_facet = element_of_facet
        bd = mesh.boundary_facets([getattr(mesh, "source_tag", 2)]) if facets is None else np.asarray(facets).reshape(-1, 2)
        self.array = SourceArray(element_of_facet, n_elements=n_elements)
        self.ids = self.array.assign(mesh, bd)
        self.n_elements = E = self.array.n_elements
        super().__init__(float_type, mesh.ndofs, E, capacity, harmonics, frequency)
        dev = self.dev
        fdm = np.asarray(mesh.facet_dofmap(bd)).reshape(bd.shape[0], (int(mesh.P) + 1) ** 2)
        if fdm.size and int(fdm.max()) >= self.ndofs:
            raise ValueError("facet dofmap entry outside the local vector")
        if detJ is None:  # as the solvers' set-up forms it
            from .solver_base import device_facet_detJ

            detJ, = device_facet_detJ(mesh, int(mesh.P), self.tdt_np, dev, [bd])
        detJ = detJ.detach().cpu().numpy() if isinstance(detJ, torch.Tensor) else np.asarray(detJ)
        dof, wgt, self.offsets = element_entries(self.ids, fdm, detJ.astype(self.tdt_np), E)
        # the area of an element is the sum of the weights the kernel multiplies with (those of the field's type), in double
        self._areas = np.add.reduceat(np.append(wgt.astype(np.float64), 0.0), self.offsets[:-1]) * (np.diff(self.offsets) > 0)
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        if dof.size == 0:  # no entries on this rank: the kernel reads none, and the C ABI takes no null list
            dof, wgt = np.zeros(1, np.int32), np.zeros(1, self.tdt_np)
        self._dof, self._wgt, self._offsets = td(dof), td(wgt), td(self.offsets)
        self.reset()

    # -- device --------------------------------------------------------------------------------------------------------
    def record(self, u, t):
        """One launch: row ``nrec`` of the series and the harmonic terms of the elements' integrals of ``u`` (device, owned + ghosts,
        ghosts current) at time ``t``."""
        from . import operators as ops

        self._check_record(u)
        ops.element_receive(u, self._dof, self._wgt, self._offsets, self._rec, self.nrec, self._hre, self._him, self.factors.row(t))
        self._recorded()

    # -- host accessors ------------------------------------------------------------------------------------------------
    def areas(self):
        """``A_e = sum wgt`` of this rank's part of every element, ``[E]`` (0 for an element without facets here)."""
        return self._areas.copy()

    def integrals(self):
        """The recorded rows as the device holds them, ``[nrec, E]``: this rank's part of ``int_{Gamma_e} u dS``."""
        if self._rec is None:
            return np.zeros((0, self.n_elements), dtype=self.tdt_np)
        return self._rec[: self.nrec].cpu().numpy()

    def harmonic_sums(self, k):
        """``sum_t S_e(t) e^{-i k w t}`` over the records, complex ``[E]``: this rank's part, not normalised."""
        h = self.factors.index(k)
        return self._hre[h].cpu().numpy() + 1j * self._him[h].cpu().numpy()

    def series(self):
        """The area-averaged series ``S_e / A_e``, ``[nrec, E]`` (fp64; one rank -- partitioned: ``merge`` / ``gather``)."""
        return merge([(self._areas, self.integrals().astype(np.float64))])

    def harmonic(self, k):
        """The complex amplitude of the k-th harmonic of the area-averaged signal, ``[E]``: ``(2 / N) sum p e^{-i k w t}`` over the N
        records, i.e. ``a e^{i phi}`` for ``p = a cos(k w t + phi)`` sampled over whole periods."""
        return merge([(self._areas, self.harmonic_sums(k))]) * (2.0 / max(self.nacc, 1))

    def gather(self, comm, values=None):
        """The area averages over the whole elements from every rank's parts (``values``: this rank's integrals, default
        ``integrals()``; elements on the last axis) through the communicator's bootstrap.  Ranks driven from one process: ``merge``."""
        from .scatterer import comm_size, gather_arrays

        values = self.integrals().astype(np.float64) if values is None else np.asarray(values)
        if comm_size(comm) == 1:
            return merge([(self._areas, values)])
        every = gather_arrays(comm, {"areas": self._areas, "values": values}, "ElementReceivers.gather", "receivers.merge")
        return merge([(z["areas"], z["values"]) for z in every])


def time_reversal(receivers_or_harmonic, harmonic=1, amplitude="uniform", duration=None, element_of_facet=None):
    """The ``SourceArray`` that fires back what the array received: ``phase_e = -arg(R_e)`` wrapped to (-pi, pi], ``R_e`` the complex
    amplitude of ``harmonic`` at element e -- an ``ElementReceivers`` (one rank: its ``harmonic(k)`` and its ``element_of_facet``) or
    the complex array ``[E]`` itself (merged over ranks; ``element_of_facet`` is then required).  ``amplitude``: ``"uniform"`` (1 for
    every element that received something) or ``"conjugate"`` (``|R_e| / max |R|``); an element that received nothing (``R_e`` zero
    or NaN) stays silent in both."""
    if amplitude not in ("uniform", "conjugate"):
        raise ValueError(f"amplitude must be 'uniform' or 'conjugate', got {amplitude!r}")
    if isinstance(receivers_or_harmonic, ElementReceivers):
        R = receivers_or_harmonic.harmonic(harmonic)
        element_of_facet = receivers_or_harmonic.element_of_facet if element_of_facet is None else element_of_facet
    else:
        R = np.asarray(receivers_or_harmonic, dtype=np.complex128).reshape(-1)
    if element_of_facet is None:
        raise ValueError("time_reversal: an array of harmonics needs element_of_facet")
    mag = np.where(np.isfinite(R), np.abs(R), 0.0)
    if R.size == 0 or not mag.max() > 0.0:
        raise ValueError("time_reversal: no element received anything")
    heard = mag > 0.0
    phi = np.where(heard, -np.angle(np.where(heard, R, 1.0)), 0.0)
    phi = np.pi - np.mod(np.pi - phi, 2.0 * np.pi)
    amp = mag / mag.max() if amplitude == "conjugate" else heard.astype(np.float64)
    return SourceArray(element_of_facet, amplitude=amp, phase=np.where(heard, phi, 0.0), duration=duration, n_elements=R.size)


def time_reversed_waveform(receivers_or_series, dt, element_of_facet=None, taper=0.0, amplitude="uniform"):
    """The ``SourceArray`` that re-emits the recorded SIGNALS reversed in time (``time_reversal`` fires one conjugate phase per element
    at one harmonic; this is the broadband form, which refocuses a pulse through a reverberating medium): element e emits row e of
    ``sources.SampledWaveform(series[::-1].T, dt, t0=0)``, i.e. ``w_e(s) = S_e(T_rec - s)`` with ``T_rec = (nrec - 1) dt`` -- an
    ``ElementReceivers`` (one rank: its ``series()`` and its ``element_of_facet``) or the merged ``[nrec, E]`` array itself
    (``element_of_facet`` is then required).  ``dt``: the recording interval.  ``amplitude``: ``"uniform"`` (each row divided by its own
    largest absolute value) or ``"recorded"`` (every row divided by the largest over all elements: the relative levels are kept).
    ``taper``: the fraction of the window, at each end, that is multiplied by a cosine ramp (0: none, at most 0.5).  An element that
    heard nothing (all zero, or NaN: no facets) gets row -1, a silent element."""
    from .sources import SampledWaveform

    if amplitude not in ("uniform", "recorded"):
        raise ValueError(f"amplitude must be 'uniform' or 'recorded', got {amplitude!r}")
    taper = float(taper)
    if not 0.0 <= taper <= 0.5:
        raise ValueError(f"taper must lie in [0, 0.5], got {taper}")
    if isinstance(receivers_or_series, ElementReceivers):
        S = receivers_or_series.series()
        element_of_facet = receivers_or_series.element_of_facet if element_of_facet is None else element_of_facet
    else:
        S = np.asarray(receivers_or_series, dtype=np.float64)
    if element_of_facet is None:
        raise ValueError("time_reversed_waveform: an array of series needs element_of_facet")
    if S.ndim != 2 or S.shape[0] < 2:
        raise ValueError(f"time_reversed_waveform: a series [nrec, E] of at least two records, got shape {S.shape}")
    nrec, E = S.shape
    finite = np.all(np.isfinite(S), axis=0)
    rows = np.where(finite[:, None], S[::-1].T, 0.0)  # [E, nrec], reversed in time
    peak = np.abs(rows).max(axis=1) if E else np.zeros(0)
    heard = peak > 0.0
    if not heard.any():
        raise ValueError("time_reversed_waveform: no element received anything")
    rows = rows / (np.where(heard, peak, 1.0)[:, None] if amplitude == "uniform" else peak.max())
    nt = int(round(taper * (nrec - 1)))
    if nt > 0:
        ramp = 0.5 * (1.0 - np.cos(np.pi * np.arange(nt) / nt))  # 0 at the end sample, below 1 at sample nt - 1
        rows[:, :nt] *= ramp
        rows[:, nrec - nt:] *= ramp[::-1]
    wf = SampledWaveform(rows, dt, t0=0.0)
    return SourceArray(element_of_facet, waveform=wf, waveform_of_element=np.where(heard, np.arange(E), -1), n_elements=E)
