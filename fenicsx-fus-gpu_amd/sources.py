"""
Phased-array sources: every source facet belongs to an element with its own amplitude factor, phase and delay, and the
array may fire a tone burst instead of a continuous wave (csrc/source_array.hpp, ``fus_facet_source_array_*``).

The solvers drive the source facets with one waveform, ``g(t) = A W(t) cos(w0 t)`` (``LinearSpectral3D.source_value``,
``WesterveltSpectral3D.source_values``).  A ``SourceArray`` assigns each source facet an element id ``e`` in ``[0, E)``
(or -1: inactive) and, with ``s = t - tau_e``,

    g_e(t) = a_e A Env(s) cos(w0 s + phi_e)          Env = W(s) (continuous wave)  or  W(s) W(D - s) (burst of duration D)

with the solvers' ramp ``W`` (4 periods).  A one-element array with ``a = 1, phi = 0, tau = 0, D = None`` is the scalar
source.  Electronic focusing, steering, phase correction through a skull and apodisation are choices of ``phi`` / ``tau`` / ``a``:

    arr = SourceArray(element_of_facet=ring_id, delay=focus_delays(centres, focus, 1500.0))
    solver = LinearSpectral3D(mesh, source=arr)          # or WesterveltSpectral3D(..., source=arr)

``element_of_facet`` is a callable from facet centroids ``[m, 3]`` to ids (what a partitioned run needs: each rank binds
its own facets and the assignment by position agrees across ranks) or an int array aligned with the rows of
``mesh.boundary_facets([source_tag])``.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib
from . import operators as ops

ALPHA = 4.0  # ramp length in periods (linear_solver.source_value, nonlinear_solver.source_values)
STAGE_WORDS = 6  # t, w0, A, f0, alpha, D  (csrc/source_array.hpp SourceStage)


def _window(s, f0, alpha=ALPHA):
    """W(s) and W'(s) (arrays), the expressions of the solvers' source terms; 0 for s <= 0."""
    s = np.asarray(s, dtype=np.float64)
    T = 1.0 / f0
    ramp = (s > 0.0) & (s < T * alpha)
    w = np.where(s >= T * alpha, 1.0, 0.0)
    dw = np.zeros_like(s)
    if ramp.any():
        sr = s[ramp]
        w[ramp] = 0.5 * (1.0 - np.cos(f0 * np.pi * sr / alpha))
        dw[ramp] = 0.5 * np.pi * f0 / alpha * np.sin(f0 * np.pi * sr / alpha)
    return w, dw


def _waveform(t, frequency, scale, amplitude, phase, delay, duration, alpha=ALPHA):
    """Host ``(g(t), dg/dt)`` of the waveform both source kinds share, one value per element / point:
    ``g = a A Env(s) cos(w0 s + phi)``, ``s = t - tau`` (the module docstring)."""
    f0 = float(frequency)
    w0 = 2.0 * np.pi * f0
    s = float(t) - delay
    env, denv = _window(s, f0, alpha)
    if duration is not None:
        w2, dw2 = _window(duration - s, f0, alpha)
        env, denv = env * w2, denv * w2 - env * dw2
    a = amplitude * float(scale)
    cs, sn = np.cos(w0 * s + phase), np.sin(w0 * s + phase)
    return env * a * cs, denv * a * cs - env * a * w0 * sn


def stencil_derivative(f, dt):
    """``df/ds`` at the samples of ``f`` [..., Nt] (interval ``dt``), fourth order: the five-point central stencil, and at the first
    two and the last two samples the one-sided five-point stencils (no zero padding: a table that does not end at 0 would get a
    derivative error that grows like 1 / dt).  Fewer than five samples leave no five-point stencil: second-order differences then
    (``Nt`` 3 or 4), the one difference quotient for ``Nt = 2``."""
    f = np.asarray(f, dtype=np.float64)
    Nt = f.shape[-1]
    if Nt < 5:
        return np.gradient(f, float(dt), axis=-1, edge_order=2 if Nt >= 3 else 1)
    d = np.empty_like(f)
    d[..., 2:-2] = (f[..., :-4] - 8.0 * f[..., 1:-3] + 8.0 * f[..., 3:-1] - f[..., 4:]) / 12.0
    d[..., 0] = (-25.0 * f[..., 0] + 48.0 * f[..., 1] - 36.0 * f[..., 2] + 16.0 * f[..., 3] - 3.0 * f[..., 4]) / 12.0
    d[..., 1] = (-3.0 * f[..., 0] - 10.0 * f[..., 1] + 18.0 * f[..., 2] - 6.0 * f[..., 3] + f[..., 4]) / 12.0
    d[..., -1] = (25.0 * f[..., -1] - 48.0 * f[..., -2] + 36.0 * f[..., -3] - 16.0 * f[..., -4] + 3.0 * f[..., -5]) / 12.0
    d[..., -2] = (3.0 * f[..., -1] + 10.0 * f[..., -2] - 18.0 * f[..., -3] + 6.0 * f[..., -4] - f[..., -5]) / 12.0
    return d / float(dt)


class SampledWaveform:
    """An arbitrary source signal per row, sampled: ``wf = SampledWaveform(samples, dt, t0=0.0, derivative=None)``.

    ``samples``: ``[R, Nt]`` (or ``[Nt]``: one row), ``R >= 1``, ``Nt >= 2``, finite; ``dt > 0``: the sample interval; ``t0``: the time
    of sample 0.  Row ``r`` defines ``w_r(s)`` on ``[t0, t0 + (Nt - 1) dt]``; outside that interval it is ZERO.  ``derivative``: ``dw/ds``
    at the samples, of the shape of ``samples``; ``None`` forms it with ``stencil_derivative`` (fourth order, one-sided at the ends).

    The interpolant is the cubic Hermite of value and derivative on each interval: C1, exact at the nodes, fourth order in the value
    and third in the derivative, which is the ``dg/dt`` the Westervelt source term needs.  With ``x = (s - t0) / dt``:

        x < 0, x > Nt - 1 or x not a number: nothing is contributed
        k = min(floor(x), Nt - 2), th = x - k        (the last node: k = Nt - 2, th = 1)
        w  = h00 w_k + h10 dt d_k + h01 w_{k+1} + h11 dt d_{k+1}
        dw = (h00' w_k + h01' w_{k+1}) / dt + h10' d_k + h11' d_{k+1}
        h00 = (1 + 2 th)(1 - th)^2,  h10 = th (1 - th)^2,  h01 = th^2 (3 - 2 th),  h11 = th^2 (th - 1)

    ``values`` is that in numpy (fp64), the arithmetic of the kernels (csrc/source_wave.hpp); ``table`` is what they read,
    ``double[R][Nt][2]``, value and derivative interleaved."""

    def __init__(self, samples, dt, t0=0.0, derivative=None):
        w = np.asarray(samples, dtype=np.float64)
        if w.ndim == 1:
            w = w[None, :]
        if w.ndim != 2 or w.shape[0] < 1:
            raise ValueError(f"samples: [R, Nt] or [Nt], got shape {np.shape(samples)}")
        if w.shape[1] < 2:
            raise ValueError(f"samples: at least two samples per row (Nt >= 2), got Nt = {w.shape[1]}")
        if not np.all(np.isfinite(w)):
            raise ValueError("samples: values must be finite")
        dt, t0 = float(dt), float(t0)
        if not (np.isfinite(dt) and dt > 0.0):
            raise ValueError(f"dt must be a positive number of seconds, got {dt}")
        if not np.isfinite(t0):
            raise ValueError(f"t0 must be finite, got {t0}")
        if derivative is None:
            d = stencil_derivative(w, dt)
        else:
            d = np.asarray(derivative, dtype=np.float64)
            if d.ndim == 1:
                d = d[None, :]
            if d.shape != w.shape:
                raise ValueError(f"derivative: the shape of samples {w.shape}, got {d.shape}")
            if not np.all(np.isfinite(d)):
                raise ValueError("derivative: values must be finite")
        self.samples, self.derivative = np.ascontiguousarray(w), np.ascontiguousarray(d)
        self.dt, self.t0 = dt, t0
        self.n_rows, self.n_samples = int(w.shape[0]), int(w.shape[1])

    @property
    def t_end(self):
        return self.t0 + (self.n_samples - 1) * self.dt

    def table(self, rows=None):
        """``double[R'][Nt][2]`` of ``rows`` (default: every row), value and derivative interleaved: what the kernels read."""
        rows = slice(None) if rows is None else np.asarray(rows, dtype=np.int64)
        return np.ascontiguousarray(np.stack([self.samples[rows], self.derivative[rows]], axis=-1))

    def values(self, s, rows=0):
        """``(w, dw)`` of row ``rows`` at time ``s`` (broadcast against each other), fp64; a row outside ``[0, R)`` is silent (zero)."""
        s, rows = np.broadcast_arrays(np.asarray(s, dtype=np.float64), np.asarray(rows, dtype=np.int64))
        Nt, dt = self.n_samples, self.dt
        x = (s - self.t0) / dt
        with np.errstate(invalid="ignore"):
            live = (x >= 0.0) & (x <= float(Nt - 1)) & (rows >= 0) & (rows < self.n_rows)
        w, dw = np.zeros(s.shape), np.zeros(s.shape)
        if live.any():
            xl, r = x[live], rows[live]
            k = np.minimum(xl.astype(np.int64), Nt - 2)
            th = xl - k
            wk, dk, wk1, dk1 = self.samples[r, k], self.derivative[r, k], self.samples[r, k + 1], self.derivative[r, k + 1]
            um = 1.0 - th
            h00, h10 = (1.0 + 2.0 * th) * (um * um), th * (um * um)
            h01, h11 = (th * th) * (3.0 - 2.0 * th), (th * th) * (th - 1.0)
            w[live] = h00 * wk + h10 * (dt * dk) + h01 * wk1 + h11 * (dt * dk1)
            d00, d10, d11 = 6.0 * th * (th - 1.0), um * (1.0 - 3.0 * th), th * (3.0 * th - 2.0)
            dw[live] = (d00 * wk - d00 * wk1) / dt + d10 * dk + d11 * dk1
        return w, dw

    @classmethod
    def from_pressure(cls, p, dt, p0, f0, t0=0.0):
        """The waveform that makes the source facets emit the surface pressure ``p`` [R, Nt] (or [Nt]), sampled every ``dt``: the
        facet source term is ``(1 / c0) dp/dt``, and the solvers' source constant is ``A = p0 w0 / c0`` (which is why today's source
        multiplies a cosine), so ``w = (dp/dt) / (p0 2 pi f0)``, with ``dp/dt`` from ``stencil_derivative``."""
        p = np.asarray(p, dtype=np.float64)
        if not np.all(np.isfinite(p)):
            raise ValueError("p: values must be finite")
        if not (float(p0) > 0.0 and float(f0) > 0.0):
            raise ValueError("p0 and f0 must be positive")
        return cls(stencil_derivative(np.atleast_2d(p), dt) / (float(p0) * 2.0 * np.pi * float(f0)), dt, t0=t0)


def _row_map(row_of, n, wf, name, what):
    """The row of the waveform per element / point, int64 [n]: ``row_of`` checked against ``[-1, R)`` (-1: silent) or, when None, row
    0 for everyone (``R == 1``) or the identity (``R == n``)."""
    R = wf.n_rows
    if row_of is None:
        if R == 1:
            return np.zeros(n, dtype=np.int64)
        if R == n:
            return np.arange(n, dtype=np.int64)
        raise ValueError(f"{name}: a waveform of {R} rows for {n} {what} needs a row per {what[:-1]} (R is neither 1 nor {n})")
    rows = np.asarray(row_of)
    if rows.shape != (n,) or not np.issubdtype(rows.dtype, np.integer):
        raise ValueError(f"{name}: one integer row per {what[:-1]} ({n}), got shape {rows.shape}, dtype {rows.dtype}")
    if rows.size and (rows.min() < -1 or rows.max() >= R):
        raise ValueError(f"{name}: rows must lie in [-1, {R}), got [{rows.min()}, {rows.max()}]")
    return rows.astype(np.int64)


def _check_waveform(wf, phase, duration):
    if not isinstance(wf, SampledWaveform):
        raise ValueError(f"waveform: a SampledWaveform, got {type(wf).__name__}")
    if duration is not None or np.any(np.asarray(phase, dtype=np.float64) != 0.0):
        raise ValueError("phase and duration belong to the analytic waveform: with waveform= they must keep their defaults")


def _sampled_values(wf, rows, t, scale, amplitude, delay):
    """Host ``(g, dg/dt)`` per element / point of a sampled source: ``g = a A w_r(t - tau)``."""
    w, dw = wf.values(float(t) - delay, rows)
    a = amplitude * float(scale)
    return a * w, a * dw


def _upload_rows(wf, rows, used):
    """The table of the rows that the elements / points ``used`` (bool mask) refer to, and ``rows`` renumbered into it (int32; an
    element that is not used, or silent, gets -1): a rank uploads the rows its own facets or points use.  A rank that uses none
    uploads row 0, which nothing refers to (the entry points want a table)."""
    live = used & (rows >= 0)
    keep = np.unique(rows[live])
    local = np.full(rows.shape, -1, dtype=np.int32)
    local[live] = np.searchsorted(keep, rows[live]).astype(np.int32)
    return wf.table(keep if keep.size else [0]), local


def facet_centroids(mesh, facets):
    """``[m, 3]`` centroids of the boundary facets ``facets`` (``(cell, local facet)`` rows): the mean of the facet's four
    vertices, from ``x_dofs`` / ``x_g`` (any mesh the solvers take: ``BoxMesh``, ``dolfinx_adaptor.ArrayMesh``)."""
    from .precompute import HEX_FACET_AXIS_SIDE

    bd = np.asarray(facets).reshape(-1, 2)
    if bd.shape[0] == 0:
        return np.zeros((0, 3))
    # vertex v = vx + 2 vy + 4 vz (precompute.tabulate_hex_p1_gradients): facet (axis, side) holds the four with bit ``axis`` = side
    verts = np.array([[v for v in range(8) if (v >> axis) & 1 == side] for axis, side in HEX_FACET_AXIS_SIDE])
    xg = np.asarray(mesh.x_g, dtype=np.float64)
    xd = np.asarray(mesh.x_dofs)
    return xg[xd[bd[:, 0][:, None], verts[bd[:, 1]]]].mean(axis=1)


def _per_element(value, E, name):
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        return np.full(E, float(a))
    if a.shape != (E,):
        raise ValueError(f"{name}: a scalar or one value per element ({E}), got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name}: values must be finite")
    return np.ascontiguousarray(a)


class SourceArray:
    """The elements of a phased array and what each facet of the source set belongs to (see the module docstring).

    ``amplitude`` / ``phase`` (radians) / ``delay`` (seconds): scalars or one value per element; ``duration``: the burst
    length ``D`` in seconds (at least two ramps, ``2 alpha / f0``, checked when bound) or ``None`` (continuous wave);
    ``n_elements``: ``E`` (default: the length of an array parameter, else the largest id + 1).

    ``waveform``: a ``SampledWaveform`` instead of the analytic form, ``g_e(t) = a_e A w_{r(e)}(t - tau_e)`` with ``dg_e/dt`` alike
    (csrc/source_wave.hpp, ``fus_facet_source_wave_*``); ``waveform_of_element``: the row ``r(e)`` per element, int [E] in ``[-1, R)``
    (-1: a silent element; default: row 0 for every element when ``R == 1``, the identity when ``R == E``).  ``phase`` and ``duration``
    belong to the analytic form and must keep their defaults then."""

    def __init__(self, element_of_facet, amplitude=1.0, phase=0.0, delay=0.0, duration=None, n_elements=None, waveform=None,
                 waveform_of_element=None):
        self.element_of_facet = element_of_facet
        if not callable(element_of_facet):
            ids = np.asarray(element_of_facet)
            if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
                raise ValueError("element_of_facet: a callable of the facet centroids or a 1-D int array")
            self.element_of_facet = ids.astype(np.int64)
        E = n_elements
        if E is None:
            lens = {np.size(v) for v in (amplitude, phase, delay) + (() if waveform_of_element is None else (waveform_of_element,))
                    if np.ndim(v) > 0}
            if len(lens) > 1:
                raise ValueError(f"per-element parameters of different lengths {sorted(lens)}")
            if lens:
                E = lens.pop()
            elif not callable(self.element_of_facet):
                E = int(self.element_of_facet.max()) + 1 if self.element_of_facet.size else 1
            else:
                E = 1
        E = int(E)
        if E < 1:
            raise ValueError(f"n_elements must be >= 1, got {E}")
        self.n_elements = E
        self.amplitude = _per_element(amplitude, E, "amplitude")
        self.phase = _per_element(phase, E, "phase")
        self.delay = _per_element(delay, E, "delay")
        if duration is not None:
            duration = float(duration)
            if not (np.isfinite(duration) and duration > 0.0):
                raise ValueError(f"duration must be a positive number of seconds or None, got {duration}")
        self.duration = duration
        self.waveform, self.waveform_of_element = waveform, None
        if waveform is not None:
            _check_waveform(waveform, phase, duration)
            self.waveform_of_element = _row_map(waveform_of_element, E, waveform, "waveform_of_element", "elements")
        elif waveform_of_element is not None:
            raise ValueError("waveform_of_element needs waveform=")

    # -- host evaluation -----------------------------------------------------------------------
    def check_duration(self, frequency, alpha=ALPHA):
        if self.duration is not None and self.duration < 2.0 * alpha / float(frequency):
            raise ValueError(f"duration {self.duration} s is shorter than the two ramps of the burst ({2.0 * alpha / float(frequency)} s)")

    def values(self, t, frequency, scale, alpha=ALPHA):
        """Host ``(g_e(t), dg_e/dt)``, ``[E]`` each, for carrier ``frequency`` and source constant ``scale`` (``A``)."""
        if self.waveform is not None:
            return _sampled_values(self.waveform, self.waveform_of_element, t, scale, self.amplitude, self.delay)
        return _waveform(t, frequency, scale, self.amplitude, self.phase, self.delay, self.duration, alpha)

    def stage_scalars(self, t, frequency, scale, alpha=ALPHA):
        """The fp64 stage block ``{t, w0, A, f0, alpha, D}`` of the kernel (``D = 0``: continuous wave)."""
        f0 = float(frequency)
        return np.array([float(t), 2.0 * np.pi * f0, float(scale), f0, float(alpha), self.duration or 0.0], dtype=np.float64)

    def assign(self, mesh, facets):
        """Element id of every row of ``facets`` (int32), validated against ``[-1, E)``."""
        bd = np.asarray(facets).reshape(-1, 2)
        if callable(self.element_of_facet):
            ids = np.asarray(self.element_of_facet(facet_centroids(mesh, bd))).reshape(-1)
            if ids.size and not np.issubdtype(ids.dtype, np.integer):
                raise ValueError("element_of_facet(centroids) must return integer ids")
        else:
            ids = self.element_of_facet
        if ids.shape != (bd.shape[0],):
            raise ValueError(f"element_of_facet: {ids.shape[0]} ids for {bd.shape[0]} source facets")
        if ids.size and (ids.min() < -1 or ids.max() >= self.n_elements):
            raise ValueError(f"element ids must lie in [-1, {self.n_elements}), got [{ids.min()}, {ids.max()}]")
        return np.ascontiguousarray(ids.astype(np.int32))

    def bind(self, mesh, facets, dtype, device, frequency=None, scale=None, coeff1=None, coeff2=None, detJ=None, dofmap=None):
        """Upload the element table for this rank's source facets ``facets`` (``mesh.boundary_facets([source_tag])``).
        ``frequency`` / ``scale``: the carrier and the source constant ``A`` of the solver; ``coeff1`` / ``coeff2`` / ``detJ``
        / ``dofmap``: the set-A tensors of the facet launch (``dofmap`` default: ``mesh.facet_dofmap(facets)``)."""
        import torch

        from . import _lib

        ids = self.assign(mesh, facets)
        if frequency is not None:
            self.check_duration(frequency)
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        if dofmap is None:
            dofmap = td(np.asarray(mesh.facet_dofmap(np.asarray(facets).reshape(-1, 2)), dtype=np.int32))
        table = rows = None
        if self.waveform is not None:  # the rows this rank's facets use
            table, rows = _upload_rows(self.waveform, self.waveform_of_element, np.bincount(ids[ids >= 0], minlength=self.n_elements) > 0)
            table, rows = td(table), td(rows)
        return BoundSourceArray(self, _lib.torch_dtype(dtype), td(ids), td(self.amplitude), td(self.phase), td(self.delay),
                                None if frequency is None else float(frequency), None if scale is None else float(scale),
                                coeff1, coeff2, detJ, dofmap, ids, table, rows)


@dataclass
class BoundSourceArray:
    """A ``SourceArray`` on the device for one rank's source facets: what ``operators.facet_source_terms`` launches with."""

    array: SourceArray
    dtype: object  # torch dtype of the field
    element_of_facet: object  # int32 [m]
    amplitude: object  # float64 [E]
    phase: object
    delay: object
    frequency: float | None
    scale: float | None
    coeff1: object = None  # T [m]: cA1 (facet_coeff1 / fc1_1)
    coeff2: object = None  # T [m] or None: cA2 (fc2_1 of the Westervelt solver)
    detJ: object = None  # T [m, n^2]
    dofmap: object = None  # int32 [m, n^2]
    ids: np.ndarray = None  # host copy of element_of_facet
    table: object = None  # float64 [R', Nt, 2] or None: the rows of ``array.waveform`` this rank uses (csrc/source_wave.hpp)
    row_of_element: object = None  # int32 [E]: the row of ``table`` per element, -1: silent or not on this rank

    @property
    def n_elements(self):
        return self.array.n_elements

    @property
    def nfacets(self):
        return int(self.element_of_facet.shape[0])

    def values(self, t):
        return self.array.values(t, self.frequency, self.scale)

    def stage_scalars(self, t):
        return self.array.stage_scalars(t, self.frequency, self.scale)

    # -- the source object of a solver (``ScalarFacetSource`` is the other) ----------------------
    stage_row = stage_scalars

    def stage_slot(self, dtype, device):
        """The stage blocks of the four stages of a captured step: fp64 for fp32 fields too."""
        import torch

        return torch.zeros((4, STAGE_WORDS), dtype=torch.float64, device=device)

    def launch(self, b, field, t=None, slot=None):
        ops.facet_source_terms(b, self, field, stage=None if slot is not None else self.stage_scalars(t), stage_dev=slot)


class ScalarFacetSource:
    """The solvers' one waveform on the source facets as a source object: what a solver asks of its source is the host row of a stage
    time (``stage_row(t)``), the zeroed device tensor [4, width] a captured step reads its four rows from (``stage_slot``), and the
    facet launch of set A together with set B (``launch(b, field, t=None, slot=None)``: the row evaluated at ``t``, or read by the
    kernel from ``slot``, one stage's row of the slot tensor; ``field`` = set B or None).  ``source_set``: set A, ``(c1, c2 or
    None, detJ, dofmap)``; ``scalars``: the solver's ``_source_scalars``, ``t -> (s1, s2)``."""

    def __init__(self, source_set, scalars):
        self.source_set, self.stage_row = source_set, scalars

    def stage_slot(self, dtype, device):
        import torch

        return torch.zeros((4, 2), dtype=dtype, device=device)

    def launch(self, b, field, t=None, slot=None):
        c1, c2, detJ, dofmap = self.source_set
        s1, s2 = (0.0, 0.0) if slot is not None else self.stage_row(t)
        ops.facet_terms(b, (c1, s1, c2, s2, detJ, dofmap), field, scalars=slot)


# -- point sources -----------------------------------------------------------------------------
class PointSources:
    """Monopole sources inside the volume, ``q_p(t) delta(x - x_p)`` (csrc/point_source.hpp, ``fus_point_source_*``): the term a
    stage's right-hand side gets is ``b[dofmap[c][ijk]] += g_p(t) Lx[i] Ly[j] Lz[k]``, the transpose of a point sensor, with the
    array's waveform per point, ``g_p(t) = a_p Env(s) cos(w0 s + phi_p)``, ``s = t - tau_p``.  The amplitude IS the monopole strength
    (the stage block's ``A`` is 1).  A virtual source at the target of a time-reversal run (receivers.py):

        solver = LinearSpectral3D(mesh, source_amplitude=0.0, point_source=PointSources(focus))

    ``points``: ``[m, 3]`` (or one point); ``amplitude`` / ``phase`` (radians) / ``delay`` (seconds): scalars or one value per point;
    ``duration``: burst length in seconds or ``None`` (continuous wave), as ``SourceArray``.

    ``waveform`` / ``waveform_of_point``: a ``SampledWaveform`` and its row per point, with the rules of ``SourceArray``:
    ``g_p(t) = a_p w_{r(p)}(t - tau_p)`` (csrc/source_wave.hpp, ``fus_point_source_wave_*``)."""

    def __init__(self, points, amplitude=1.0, phase=0.0, delay=0.0, duration=None, waveform=None, waveform_of_point=None):
        pts = np.asarray(points, dtype=np.float64)
        if pts.ndim == 1 and pts.size == 3:
            pts = pts[None, :]
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError(f"points: [m, 3] points, got shape {pts.shape}")
        if not np.all(np.isfinite(pts)):
            raise ValueError("points: coordinates must be finite")
        self.points = np.ascontiguousarray(pts)
        m = self.npoints = int(pts.shape[0])
        self.amplitude = _per_element(amplitude, m, "amplitude")
        self.phase = _per_element(phase, m, "phase")
        self.delay = _per_element(delay, m, "delay")
        if duration is not None:
            duration = float(duration)
            if not (np.isfinite(duration) and duration > 0.0):
                raise ValueError(f"duration must be a positive number of seconds or None, got {duration}")
        self.duration = duration
        self.waveform, self.waveform_of_point = waveform, None
        if waveform is not None:
            _check_waveform(waveform, phase, duration)
            self.waveform_of_point = _row_map(waveform_of_point, m, waveform, "waveform_of_point", "points")
        elif waveform_of_point is not None:
            raise ValueError("waveform_of_point needs waveform=")

    check_duration = SourceArray.check_duration
    stage_scalars = SourceArray.stage_scalars

    def values(self, t, frequency, scale=1.0, alpha=ALPHA):
        """Host ``(g_p(t), dg_p/dt)``, ``[m]`` each, as ``SourceArray.values`` (a one-point source equals a one-element array)."""
        if self.waveform is not None:
            return _sampled_values(self.waveform, self.waveform_of_point, t, scale, self.amplitude, self.delay)
        return _waveform(t, frequency, scale, self.amplitude, self.phase, self.delay, self.duration, alpha)

    def setup(self, mesh, locator=None):
        """This rank's ``sensors.SensorSetup`` of the points: those that lie in one of its cells, sorted by cell."""
        from .sensors import sensor_setup

        return sensor_setup(mesh, self.points, locator)

    def bind(self, mesh, dtype, device, frequency, comm=None, claim=None, setup=None, locator=None):
        """Locate the points in this rank's cells (``sensors.sensor_setup``) and upload the tables of those it injects.  Every point
        is injected by exactly ONE rank, the lowest that holds it (the rule of ``sensors.merge``): ranks in different processes agree
        through one gather over ``comm`` here; ranks driven from one process are handed ``claim``, this rank's row of
        ``claim_points`` (all ranks' set-ups).  On one rank a point outside the mesh is a ``ValueError``."""
        import torch

        from . import _lib
        from .scatterer import comm_size, gather_arrays

        self.check_duration(frequency)
        su = setup if setup is not None else self.setup(mesh, locator)
        if claim is None:
            if comm_size(comm) == 1:
                if su.point_ids.size != self.npoints:
                    lost = np.setdiff1d(np.arange(self.npoints), su.point_ids)
                    raise ValueError(f"point source(s) {lost.tolist()} lie outside the mesh")
                claim = np.ones(self.npoints, dtype=bool)
            else:
                every = gather_arrays(comm, {"ids": su.point_ids}, "PointSources.bind", "claim=claim_points(setups, npoints)[rank]")
                claim = claim_points([z["ids"] for z in every], self.npoints)[int(comm.rank)]
        claim = np.asarray(claim, dtype=bool)
        if claim.shape != (self.npoints,):
            raise ValueError(f"claim: one flag per point ({self.npoints}), got shape {claim.shape}")
        keep = claim[su.point_ids]  # device order stays sorted by cell
        ids = su.point_ids[keep]
        n = int(mesh.P) + 1
        if su.rows.size and int(su.rows.max()) >= int(mesh.ndofs):
            raise ValueError("dofmap row outside the local vector")
        ft = np.dtype(dtype)
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        return BoundPointSources(self, _lib.torch_dtype(dtype), int(mesh.P), int(mesh.ndofs), ids, td(su.cell_index[keep].astype(np.int32)),
                                 td(su.rows.astype(np.int32).reshape(-1, n**3)), td(su.weights[keep].astype(ft).reshape(-1, 3, n)),
                                 td(self.amplitude[ids]), td(self.phase[ids]), td(self.delay[ids]), float(frequency),
                                 *self._bind_waveform(ids, td))

    def _bind_waveform(self, ids, td):
        """``(table, row_of_point)`` on the device for the points ``ids`` this rank injects (device order); Nones without a waveform."""
        if self.waveform is None:
            return None, None
        table, rows = _upload_rows(self.waveform, self.waveform_of_point[ids], np.ones(ids.size, dtype=bool))
        return td(table), td(rows)


def claim_points(per_rank, npoints):
    """Which rank injects which point: ``per_rank`` holds, in rank order, each rank's ``SensorSetup`` (or its ``point_ids``); returns one
    bool row ``[npoints]`` per rank, the LOWEST rank that holds a point claiming it (``sensors.merge``'s rule).  A point that no rank
    holds is a ``ValueError``: it would be dropped silently otherwise."""
    owner = np.full(int(npoints), -1, dtype=np.int64)
    for r in reversed(range(len(per_rank))):  # the lowest rank writes last
        ids = np.asarray(getattr(per_rank[r], "point_ids", per_rank[r]), dtype=np.int64).reshape(-1)
        owner[ids] = r
    if np.any(owner < 0):
        raise ValueError(f"point source(s) {np.nonzero(owner < 0)[0].tolist()} lie outside the mesh")
    return [owner == r for r in range(len(per_rank))]


@dataclass
class BoundPointSources:
    """``PointSources`` on the device for one rank: what ``operators.point_source_terms`` launches with."""

    sources: PointSources
    dtype: object  # torch dtype of the field
    P: int
    ndofs: int  # length of the local vector the rows index
    point_ids: np.ndarray  # int64 [m]  the points this rank injects (indices into the caller's list, device order)
    cells: object  # int32 [m]  row of ``rows`` per point
    rows: object  # int32 [k, n^3]  dofmap rows of the cells that hold a located point
    weights: object  # T [m, 3, n]
    amplitude: object  # float64 [m]
    phase: object
    delay: object
    frequency: float
    table: object = None  # float64 [R', Nt, 2] or None: the rows of ``sources.waveform`` this rank's points use
    row_of_point: object = None  # int32 [m]: the row of ``table`` per point (device order), -1: silent

    @property
    def npoints(self):
        return int(self.point_ids.size)

    def values(self, t):
        g, dg = self.sources.values(t, self.frequency)
        return g[self.point_ids], dg[self.point_ids]

    def stage_scalars(self, t):
        """The fp64 stage block ``{t, w0, A = 1, f0, alpha, D}`` of the kernel."""
        return self.sources.stage_scalars(t, self.frequency, 1.0)

    # -- a stage term of a solver (solver_base): placed after the facet launch, before the reverse scatter of b (a point's cell may
    # hold ghost dofs) ----------------------------------------------------------------------------
    capturable = False
    refusal = ("a solver with point_source= cannot be replayed from a captured graph (the point sources' "
               "stage time is a host argument of their launch)")

    def bind(self, solver, mass):
        pass  # bound where the solver was constructed: nothing here waits for the mass

    def launch(self, b, u_n, v_n, t):
        """b[dofmap[c][ijk]] += g_p(t) Lx[i] Ly[j] Lz[k] over this rank's points."""
        if t is None:
            raise _lib.FusGpuError("point sources take their stage time from the host: a step with a point source cannot be captured")
        ops.point_source_terms(b, self, self.stage_scalars(t))


# -- geometry helpers --------------------------------------------------------------------------
def _points(a, name):
    p = np.asarray(a, dtype=np.float64)
    if p.ndim == 1 and p.size == 3:
        p = p[None, :]
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"{name}: [E, 3] points, got shape {p.shape}")
    return p


def focus_delays(centres, focus, c):
    """Delays that focus the elements at ``centres`` [E, 3] on ``focus`` through a medium of speed ``c``: the farthest element
    fires first (delay 0) and every wavefront reaches the focus at the same time, ``tau_e = (max_j d_j - d_e) / c``."""
    d = np.linalg.norm(_points(centres, "centres") - np.asarray(focus, dtype=np.float64).reshape(1, 3), axis=1)
    return (d.max() - d) / float(c)


def focus_phases(centres, focus, c, f):
    """The continuous-wave equivalent of ``focus_delays`` at frequency ``f``: ``phi_e = -2 pi f tau_e``, wrapped to (-pi, pi]."""
    phi = -2.0 * np.pi * float(f) * focus_delays(centres, focus, c)
    return np.pi - np.mod(np.pi - phi, 2.0 * np.pi)


def steer_delays(centres, direction, c):
    """Delays that steer a plane wave along ``direction``: ``tau_e = (x_e . k - min_j x_j . k) / c``, k the unit direction."""
    k = np.asarray(direction, dtype=np.float64).reshape(3)
    nk = np.linalg.norm(k)
    if nk == 0.0:
        raise ValueError("direction must be non-zero")
    proj = _points(centres, "centres") @ (k / nk)
    return (proj - proj.min()) / float(c)


def element_centres(mesh, facets, ids):
    """``[E, 3]`` centre of each element on ONE rank: the mean of its facets' centroids (E = largest id + 1; NaN for an element
    without facets).  A partitioned run computes the centres from the global layout instead."""
    ids = np.asarray(ids).reshape(-1)
    cen = facet_centroids(mesh, facets)
    if cen.shape[0] != ids.size:
        raise ValueError(f"{ids.size} ids for {cen.shape[0]} facets")
    E = int(ids.max()) + 1 if ids.size else 0
    out = np.full((E, 3), np.nan)
    act = ids >= 0
    cnt = np.bincount(ids[act], minlength=E).astype(np.float64)
    for a in range(3):
        s = np.bincount(ids[act], weights=cen[act, a], minlength=E)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, a] = np.where(cnt > 0, s / np.maximum(cnt, 1), np.nan)
    return out


def grid_elements(ny, nz, y_range, z_range):
    """``element_of_facet`` callable of a rectangular ``ny x nz`` split of a face normal to x: element ``j nz + k`` holds the
    facets whose centroid lies in cell (j, k) of the ``y_range`` x ``z_range`` grid."""
    (y0, y1), (z0, z1) = y_range, z_range

    def ids(cen):
        j = np.clip(np.floor((cen[:, 1] - y0) / (y1 - y0) * ny), 0, ny - 1).astype(np.int64)
        k = np.clip(np.floor((cen[:, 2] - z0) / (z1 - z0) * nz), 0, nz - 1).astype(np.int64)
        return j * nz + k

    return ids


def grid_centres(ny, nz, x, y_range, z_range):
    """``[ny nz, 3]`` centres of the elements of ``grid_elements`` on the plane ``x``."""
    (y0, y1), (z0, z1) = y_range, z_range
    yc = y0 + (np.arange(ny) + 0.5) * (y1 - y0) / ny
    zc = z0 + (np.arange(nz) + 0.5) * (z1 - z0) / nz
    Y, Z = np.meshgrid(yc, zc, indexing="ij")
    return np.stack([np.full(Y.size, float(x)), Y.reshape(-1), Z.reshape(-1)], axis=1)
