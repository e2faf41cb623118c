"""
Which steps of an RK4 run are recorded (``rk4_steps``, ``record_times``) and the harmonic factors of those steps on the device
(``HarmonicFactors``): the host side that ``sensors.PointSensors``, ``receivers.ElementReceivers`` and
``field_monitor.FieldMonitor`` share; the first two also their life cycle (``SeriesRecorder``).

A recorder's kernel reads the 2H factors of its step from device memory.  A host->device copy ordered between the launches of a
step costs more than the recorder's launch, so a time loop announces its steps first (``expect_steps`` -> ``plan``: one pinned
table, one copy); a record at any other time takes a row of a small pinned ring.  Nothing here imports torch before it is used.
"""

from __future__ import annotations

from itertools import islice

import numpy as np

_RING = 64  # pinned host rows of off-plan factors in flight (a row is waited for only when the ring comes round to it)


def rk4_steps(start_time, final_time, dt, max_steps=None):
    """``(t, dt)`` of every step of ``rk4(start_time, final_time, dt, max_steps)``: its start and its length, the last step
    shortened to end at ``final_time``.  A step ends at ``t + dt``: ``HarmonicFactors.row`` matches the recording times against
    those sums bitwise."""
    t, tf, step = float(start_time), float(final_time), 0
    while t < tf and (max_steps is None or step < max_steps):
        dt = min(dt, tf - t)
        yield t, dt
        t += dt
        step += 1


def record_times(start_time, final_time, dt, max_steps=None, record_from=None, limit=None):
    """The end times of the steps an ``rk4(start_time, final_time, dt, max_steps)`` call records: those of ``rk4_steps`` that end
    after ``record_from`` (the sums ``t + dt`` the time loop forms, bitwise), the first ``limit`` of them where one is given."""
    rf = -np.inf if record_from is None else float(record_from)
    return list(islice((t + h for t, h in rk4_steps(start_time, final_time, dt, max_steps) if t + h > rf), limit))


def coefficient_rows(harmonics, omega, times):
    """The per-step factors of the harmonic accumulators, a row per time: ``[cos(k w t), -sin(k w t)]`` for each ``k``
    ([len(times), 2H]), so that the accumulators hold ``sum_t p(t) e^{-i k w t}``."""
    k = np.asarray(harmonics, dtype=np.float64).reshape(-1)
    ph = (k * float(omega))[None, :] * np.asarray(times, dtype=np.float64)[:, None]
    return np.ascontiguousarray(np.stack([np.cos(ph), -np.sin(ph)], axis=2).reshape(ph.shape[0], -1))


def harmonic_coefficients(harmonics, omega, t):
    """``coefficient_rows`` of the one time ``t``: [2H]."""
    return coefficient_rows(harmonics, omega, [float(t)])[0]


class HarmonicFactors:
    """The factors of the multiples ``harmonics`` of ``frequency`` on the current device, a row [2H] per record (``row``).  A set
    without harmonics holds nothing and hands out ``None``."""

    def __init__(self, harmonics, frequency):
        self.harmonics = tuple(int(k) for k in harmonics)
        if self.harmonics and frequency is None:
            raise ValueError("harmonics need the fundamental frequency")
        self.omega = 2.0 * np.pi * float(frequency) if frequency is not None else None
        self._plan_t, self._plan_i, self._table, self._table_host, self._table_ev = [], 0, None, None, None
        if self.harmonics:
            import torch

            self._ring = torch.zeros((_RING, 2 * len(self.harmonics)), dtype=torch.float64).pin_memory()
            self._coef = self._ring[0].to(torch.device("cuda", torch.cuda.current_device()))  # the off-plan row the kernel reads
            self._ring_ev = [None] * _RING
            self._ri = 0

    @property
    def planned_times(self):
        """The times of the current plan, handed out or not."""
        return np.asarray(self._plan_t, dtype=np.float64)

    @property
    def planned_left(self):
        """How many planned rows ``row`` has not handed out yet."""
        return len(self._plan_t) - self._plan_i

    def index(self, k):
        """The accumulator row of harmonic ``k``."""
        if k not in self.harmonics:
            raise ValueError(f"harmonic {k} is not accumulated (harmonics={self.harmonics})")
        return self.harmonics.index(k)

    def plan_steps(self, start_time, final_time, dt, max_steps=None, record_from=None, limit=None):
        """``plan`` the steps an ``rk4(start_time, final_time, dt, max_steps)`` call records (``record_times``)."""
        self.plan(record_times(start_time, final_time, dt, max_steps, record_from, limit))

    def plan(self, times):
        """Upload, in one copy, the rows of ``times``: the records to come, in their order.  Replaces the previous plan."""
        if not self.harmonics:
            return
        import torch

        if self._table_ev is not None:
            self._table_ev.synchronize()  # the previous table's host rows: copied long ago, normally
        self._plan_t, self._plan_i = [float(t) for t in times], 0  # a list: ``row`` compares one Python float per record
        self._table = self._table_host = self._table_ev = None
        if self._plan_t:
            self._table_host = torch.from_numpy(coefficient_rows(self.harmonics, self.omega, self._plan_t)).pin_memory()
            self._table = self._table_host.to(self._coef.device, non_blocking=True)
            self._table_ev = torch.cuda.Event()
            self._table_ev.record()

    def row(self, t):
        """The device row [2H] of a record at time ``t``, for a launch on the current stream before the next call: the next planned
        row if its time equals ``t`` bitwise, otherwise this time's factors through a pinned ring row (reused once its copy has
        run) into the one off-plan row."""
        if not self.harmonics:
            return None
        i = self._plan_i
        if i < len(self._plan_t) and self._plan_t[i] == t:
            self._plan_i = i + 1
            return self._table[i]
        import torch

        k = self._ri
        self._ri = (k + 1) % _RING
        if self._ring_ev[k] is not None:
            self._ring_ev[k].synchronize()
        self._ring[k].copy_(torch.from_numpy(harmonic_coefficients(self.harmonics, self.omega, t)))
        self._coef.copy_(self._ring[k], non_blocking=True)
        self._ring_ev[k] = torch.cuda.Event()
        self._ring_ev[k].record()
        return self._coef


SERIES_LESS_STEPS = 1 << 16  # the most steps a recorder without a series (never full) plans factors for in one rk4 call


class SeriesRecorder:
    """What the two series recorders share (``sensors.PointSensors``, ``receivers.ElementReceivers``): a series of ``capacity`` rows of
    ``width`` values in the field's type, the harmonic accumulators [H, width] (fp64) with their factors, and the counters.  A
    subclass launches in ``record`` between ``_check_record(u)`` and ``_recorded()``."""

    def __init__(self, float_type, ndofs, width, capacity, harmonics, frequency):
        import torch

        from . import _lib

        self._lib = _lib
        self.ndofs = int(ndofs)
        self.tdt_np, self.tdt = np.dtype(float_type), _lib.torch_dtype(float_type)
        self.capacity = int(capacity)
        if self.capacity < 0:
            raise ValueError("capacity must be >= 0")
        self.factors = HarmonicFactors(harmonics, frequency)
        self.harmonics, self.omega = self.factors.harmonics, self.factors.omega
        self.dev = dev = torch.device("cuda", torch.cuda.current_device())
        H = len(self.harmonics)
        self._rec = torch.zeros((self.capacity, width), dtype=self.tdt, device=dev) if self.capacity else None
        self._hre = torch.empty((H, width), dtype=torch.float64, device=dev) if H else None
        self._him = torch.empty((H, width), dtype=torch.float64, device=dev) if H else None

    def reset(self):
        """Clear the series and the accumulators."""
        self.nrec = 0  # rows written to the series
        self.nacc = 0  # records accumulated into the harmonics (and whatever ``_reset_more`` clears)
        if self._hre is not None:
            self._hre.zero_()
            self._him.zero_()
        self._reset_more()

    def _reset_more(self):
        pass

    @property
    def full(self):
        """True once every row of the series is written (a set without a series is never full)."""
        return self.capacity > 0 and self.nrec >= self.capacity

    def expect_steps(self, start_time, final_time, dt, max_steps=None, record_from=None):
        """Upload, in one copy, the harmonic factors of every step an ``rk4(start_time, final_time, dt, max_steps)`` call
        will record (``record_times``: the steps that end after ``record_from``, while the series has room);
        ``record`` then reads them from that table.  The solvers call this at the start of ``rk4``."""
        room = self.capacity - self.nrec if self.capacity else SERIES_LESS_STEPS
        self.factors.plan_steps(start_time, final_time, dt, max_steps, record_from, limit=room)

    def _check_field(self, u):
        self._lib.require_device_tensor(u, self.tdt, "u")
        if u.numel() < self.ndofs:
            raise ValueError(f"u: {u.numel()} values, the mesh has {self.ndofs} local dofs")

    def _check_record(self, u):
        self._check_field(u)
        if self.full:
            raise ValueError(f"record: the series is full ({self.capacity} rows)")

    def _recorded(self):
        if self._rec is not None:
            self.nrec += 1
        self.nacc += 1
