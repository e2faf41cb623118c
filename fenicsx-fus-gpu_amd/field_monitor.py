"""
Full-field monitors: running peak, mean-square and harmonic maps over the owned dofs, accumulated on the device after every
recorded time step (csrc/field_monitor.hpp, ``fus_field_accumulate_*``), and the maps derived from them.

The reference gets its last-period maps by copying the whole field to the host at every step of its collection window and
post-processing the dumps there (cuda/demo_nonlinear_bowl.py:662-680, cuda/demo_linear_piston.py).  ``sensors.PointSensors``
does this on the device for a list of points; a ``FieldMonitor`` does it for every owned dof, one streaming launch per step:

    m = FieldMonitor(solver.nlocal, np.float64, peak=True, mean_square=("u", "v"), harmonics=(1, 2), frequency=f0)
    solver.rk4(t0, tf, dt, monitor=m, record_from=tf - period)
    m.peak(), m.mean_square("v"), m.harmonic_amplitude(2)      # device tensors [nlocal]: the caller decides what to copy

Which steps are recorded and their harmonic factors on the device come from ``recording.py``, as for the sensors: no record blocks
the host.

``v = dp/dt`` is not observable mid-run otherwise (the fused step keeps it in ``v0``); its mean square is what the absorbed power
density of the Westervelt model needs, ``q = delta / (rho c^4) <(dp/dt)^2>`` (``heat_deposition``; ``2 alpha I`` for a harmonic
wave).  ``focus`` finds the maximum of a map and the volume above a fraction of it.
"""

from __future__ import annotations

import numpy as np

from .recording import HarmonicFactors, record_times  # noqa: F401  (record_times: re-exported)

MAX_HARMONICS = 4  # csrc/field_monitor.hpp: the harmonic count is a template parameter of the kernel


class FieldMonitor:
    """Accumulators over the owned dofs ``[0, nlocal)`` of a field of ``float_type``.

    ``peak``: running max / min of u; ``mean_square``: any of ``"u"``, ``"v"`` (sums of squares, fp64); ``harmonics``: up to
    four multiples ``k`` of ``frequency`` whose complex amplitudes ``sum_t u(t) e^{-i k w t}`` are accumulated (fp64)."""

    def __init__(self, nlocal, float_type=np.float64, peak=False, mean_square=(), harmonics=(), frequency=None):
        import torch

        from . import _lib

        self._lib = _lib
        self.nlocal = int(nlocal)
        if self.nlocal < 0:
            raise ValueError("nlocal must be >= 0")
        self.tdt_np = np.dtype(float_type)
        self.tdt = _lib.torch_dtype(float_type)
        self.with_peak = bool(peak)
        ms = (mean_square,) if isinstance(mean_square, str) else tuple(mean_square)
        if any(w not in ("u", "v") for w in ms):
            raise ValueError(f"mean_square: any of 'u', 'v', got {ms}")
        self.squares = tuple(w for w in ("u", "v") if w in ms)
        harmonics = tuple(harmonics)
        if len(harmonics) > MAX_HARMONICS:
            raise ValueError(f"at most {MAX_HARMONICS} harmonics per monitor, got {len(harmonics)}")
        self.factors = HarmonicFactors(harmonics, frequency)
        self.harmonics, self.omega = self.factors.harmonics, self.factors.omega
        dev = torch.device("cuda", torch.cuda.current_device())
        self.dev = dev
        n, H = self.nlocal, len(self.harmonics)
        self.npad = n + (n & 1)  # even: every row of hre / him starts 16-byte aligned
        # never filled: the first record of a window WRITES them (``init``)
        self._pmax = torch.empty(n, dtype=self.tdt, device=dev) if peak else None
        self._pmin = torch.empty(n, dtype=self.tdt, device=dev) if peak else None
        self._usq = torch.empty(n, dtype=torch.float64, device=dev) if "u" in self.squares else None
        self._vsq = torch.empty(n, dtype=torch.float64, device=dev) if "v" in self.squares else None
        self._hre = torch.empty((H, self.npad), dtype=torch.float64, device=dev) if H else None
        self._him = torch.empty((H, self.npad), dtype=torch.float64, device=dev) if H else None
        self._fn = getattr(_lib.load(), f"fus_field_accumulate_{_lib.suffix(self.tdt)}")
        self.nacc = 0

    def reset(self):
        """Start a new window: the next record overwrites every accumulator (no device work here)."""
        self.nacc = 0

    def expect_steps(self, start_time, final_time, dt, max_steps=None, record_from=None):
        """Upload, in one copy, the harmonic factors of every step an ``rk4(start_time, final_time, dt, max_steps)`` call will
        record (``recording.record_times``: the steps that end after ``record_from``), as ``PointSensors.expect_steps`` does."""
        self.factors.plan_steps(start_time, final_time, dt, max_steps, record_from)

    def record(self, u, v=None, t=0.0):
        """One launch: the owned dofs of ``u`` (and ``v``, for its mean square) at time ``t`` into every accumulator."""
        self._lib.require_device_tensor(u, self.tdt, "u")
        if u.numel() < self.nlocal:
            raise ValueError(f"u: {u.numel()} values, the monitor covers {self.nlocal} owned dofs")
        if self._vsq is not None:
            if v is None:
                raise ValueError("record: this monitor accumulates the mean square of v: pass v")
            self._lib.require_device_tensor(v, self.tdt, "v")
            if v.numel() < self.nlocal:
                raise ValueError(f"v: {v.numel()} values, the monitor covers {self.nlocal} owned dofs")
        coef, H = self.factors.row(t), len(self.harmonics)
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        self._lib.check(
            self._fn(ptr(u), ptr(v) if self._vsq is not None else None, self.nlocal, ptr(self._pmax), ptr(self._pmin), ptr(self._usq),
                     ptr(self._vsq), ptr(self._hre), ptr(self._him), self.npad, ptr(coef), H, int(self.nacc == 0),
                     self._lib.stream_ptr()),
            "fus_field_accumulate",
        )
        self.nacc += 1

    # -- the maps (device tensors over the owned dofs) -----------------------------------------------------------------------
    def _recorded(self, what):
        if self.nacc == 0:
            raise ValueError(f"{what}: nothing recorded since the last reset")

    def peak(self):
        """``(max, min)`` of u over the records, dtype of the field."""
        if self._pmax is None:
            raise ValueError("this monitor keeps no peaks (peak=False)")
        self._recorded("peak")
        return self._pmax, self._pmin

    def mean_square(self, which="u"):
        """``<u^2>`` or ``<v^2>`` over the records (fp64)."""
        acc = {"u": self._usq, "v": self._vsq}.get(which)
        if acc is None:
            raise ValueError(f"mean square of {which!r} is not accumulated (mean_square={self.squares})")
        self._recorded("mean_square")
        return acc / float(self.nacc)

    def _harmonic(self, k):
        h = self.factors.index(k)
        self._recorded("harmonic")
        return self._hre[h, : self.nlocal], self._him[h, : self.nlocal]

    def harmonic_amplitude(self, k):
        """``(2 / N) |sum u e^{-i k w t}|`` over the N records: the amplitude of the k-th harmonic, exact for a periodic field
        sampled at N equal steps over one period."""
        import torch

        re, im = self._harmonic(k)
        return torch.hypot(re, im) * (2.0 / self.nacc)

    def harmonic_phase(self, k):
        """The phase ``phi`` of the k-th harmonic ``A cos(k w t + phi)``."""
        import torch

        re, im = self._harmonic(k)
        return torch.atan2(im, re)

    def heat_deposition(self, solver):
        return heat_deposition(self, solver)

    def intensity(self, solver):
        from .intensity import intensity

        return intensity(self, solver)

    def radiation_force(self, solver):
        from .intensity import radiation_force

        return radiation_force(self, solver)

    @staticmethod
    def focus(field, solver, level=0.5, comm=None):
        return focus(field, solver, level, comm)

    @staticmethod
    def merge_focus(records):
        return merge_focus(records)


# -- derived maps: compositions of the existing operators, once per run ------------------------------------------------------
def lumped_mass_schedule(solver, cell_constants):
    """Generator: ``diag(M(c)) = M(c) 1`` over the owned dofs (fp64), assembled with the solver's cell mass operator and, on a
    partitioned mesh, its reverse exchange (a ``yield`` after posting, as the solvers' schedules).  Returns the tensor."""
    import torch

    from . import operators as ops

    c = torch.from_numpy(np.ascontiguousarray(np.asarray(cell_constants, dtype=solver.tdt_np))).to(solver.dev)
    ones = torch.empty(solver.ndofs, dtype=solver.tdt, device=solver.dev)
    out = torch.zeros(solver.ndofs, dtype=solver.tdt, device=solver.dev)
    ops.fill(1.0, ones)
    solver.mass_cell(ones, c, out, solver.detJ, solver.dofmap)
    if solver.halo is not None:
        wk = solver.halo.rev.begin(out)
        yield "reverse"
        solver.halo.rev.end(out, wk)
    return out[: solver.nlocal].to(torch.float64)


def dof_volumes_schedule(solver):
    """Generator: ``vol = M(1) 1``, the volume each owned dof stands for (kept on the solver once formed)."""
    vol = getattr(solver, "_dof_volumes", None)
    if vol is None:
        vol = yield from lumped_mass_schedule(solver, np.ones(solver.mesh.ncells))
        solver._dof_volumes = vol
    return vol


def dof_volumes(solver):
    from .solver_base import run_schedule

    return run_schedule(dof_volumes_schedule(solver))


def heat_deposition_schedule(monitor, solver):
    """Generator form of ``heat_deposition`` for a driver that advances several ranks from one process."""
    for name in ("delta_cells", "rho_cells", "c_cells"):
        if not hasattr(solver, name):
            raise ValueError(f"heat_deposition: the solver keeps no per-cell {name} (a WesterveltSpectral3D does)")
    kappa = solver.delta_cells / solver.rho_cells / solver.c_cells**4
    vsq = monitor.mean_square("v")
    mk = yield from lumped_mass_schedule(solver, kappa)
    vol = yield from dof_volumes_schedule(solver)
    return mk * vsq / vol


def heat_deposition(monitor, solver):
    """The absorbed power density ``q = M(kappa) <v^2> / M(1) 1`` with ``kappa = delta / (rho c^4)`` per cell: the lumped-mass
    projection of ``kappa <(dp/dt)^2>``, well defined where the materials jump between cells (with GLL collocation
    ``M(kappa) x = diag(M(kappa) 1) x``).  A solver with a nodal medium (``nodal_medium=``) keeps the per-cell MEANS of its nodal
    rho and c in ``rho_cells`` / ``c_cells``: those are the values seen here.  Device tensor [nlocal], fp64."""
    from .solver_base import run_schedule

    return run_schedule(heat_deposition_schedule(monitor, solver))


def _focus_local(field, solver, level, vol):
    import torch

    n = solver.nlocal
    f = field[:n].to(torch.float64)
    if n == 0:
        return {"max": -np.inf, "dof": -1, "rank": _rank(solver), "position": None, "level": float(level), "volume": 0.0,
                "values": f, "volumes": vol}
    dof = int(torch.argmax(f).item())
    fmax = float(f[dof].item())
    keep = f >= level * fmax
    pos = None
    if hasattr(solver.mesh, "dof_coordinates"):
        pos = tuple(float(x) for x in np.asarray(solver.mesh.dof_coordinates())[dof])
    return {"max": fmax, "dof": dof, "rank": _rank(solver), "position": pos, "level": float(level),
            "volume": float(vol[keep].sum().item()), "values": f[keep], "volumes": vol[keep]}


def _rank(solver):
    return int(getattr(solver.comm, "rank", 0)) if solver.comm is not None else 0


def focus(field, solver, level=0.5, comm=None):
    """The global maximum of the map ``field`` (device tensor over the owned dofs), its owned dof, rank and position (where the
    mesh has ``dof_coordinates()``) and the volume where ``field >= level * max`` (``sum vol[d]``, ``vol = M(1) 1``): a dict
    ``max, dof, rank, position, level, volume``.  Torch reductions on the device.  ``comm``: reduce over its ranks through the
    bootstrap's ``allgather_bytes``, as ``PointSensors.gather``; without it the record is this rank's and also carries the
    candidates of the global volume (``values``, ``volumes`` of the dofs above ITS threshold) for ``merge_focus``."""
    from .scatterer import comm_size, gather_arrays

    vol = dof_volumes(solver)
    rec = _focus_local(field, solver, level, vol)
    if comm_size(comm) == 1:
        return rec

    def gather(d):
        return gather_arrays(comm, {k: np.asarray(v, dtype=np.float64) for k, v in d.items()}, "focus", "merge_focus")

    pos = rec["position"] if rec["position"] is not None else (np.nan,) * 3
    every = gather({"max": rec["max"], "dof": rec["dof"], "rank": rec["rank"], "position": pos})
    best = max(every, key=lambda r: (float(r["max"]), -int(r["rank"])))
    gmax = float(best["max"])
    f = field[: solver.nlocal]
    mine = float(vol[f >= level * gmax].sum().item()) if solver.nlocal else 0.0
    total = sum(float(r["volume"]) for r in gather({"volume": mine}))
    p = tuple(float(x) for x in best["position"])
    return {"max": gmax, "dof": int(best["dof"]), "rank": int(best["rank"]), "position": None if np.isnan(p[0]) else p,
            "level": float(level), "volume": total, "values": None, "volumes": None}


def merge_focus(records):
    """The focus over several ranks' ``focus`` records (ranks driven from one process): the largest maximum (the lowest rank
    among equals) and the volume of the candidates at or above ``level`` times it."""
    records = list(records)
    if not records:
        raise ValueError("merge_focus: no records")
    level = float(records[0]["level"])
    if any(float(r["level"]) != level for r in records):
        raise ValueError("merge_focus: records of different levels")
    best = max(records, key=lambda r: (float(r["max"]), -int(r["rank"])))
    gmax, total = float(best["max"]), 0.0
    for r in records:
        vals, vols = r["values"], r["volumes"]
        if vals is None or vols is None:
            raise ValueError("merge_focus: a record without its candidates (already reduced over ranks)")
        keep = vals >= level * gmax
        total += float(vols[keep].sum())
    return {"max": gmax, "dof": int(best["dof"]), "rank": int(best["rank"]), "position": best["position"], "level": level,
            "volume": total, "values": None, "volumes": None}
