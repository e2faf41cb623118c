"""
Pennes bioheat solver with CEM43 thermal dose on the mesh, dof numbering and partition of the acoustic solvers: what a
sonication does to tissue, from the absorbed power density ``field_monitor.heat_deposition`` leaves on the device.

    M(rho C) dT/dt = -K(k) T - M(w_b rho_b C_b)(T - T_a) + g(t) M(1) q          T in deg C, natural (insulated) boundaries

With GLL collocation every mass is diagonal, so per owned dof

    dT/dt = minv b - pr (T - T_a) + g(t) s        b = -K(k) T,  minv = 1 / M(rho C) 1,  pr = M(w_b rho_b C_b) 1 minv,  s = M(1) 1 q minv

``minv``, ``pr``, ``s`` are formed once (each lumped vector reverse-scattered on a partitioned mesh); dofs of the facets tagged
``fixed_tags`` get ``minv = pr = s = 0`` and keep their initial value.  Time stepping is classical RK4: per stage one planned
stiffness apply with the per-cell coefficient ``-k`` (next to a halo through ``HaloApply.apply_schedule``) and one streaming
vector pass (csrc/bioheat.hpp, ``fus_bioheat_stage_*``), whose last stage also updates the thermal dose and the peak temperature
from the step's end temperature -- the rule of k-Wave's kWaveDiffusion:

    cem43 += (dt / 60) R^(43 - T),  R = 0.5 for T >= 43, 0.25 below  (minutes, fp64)          tmax = max(tmax, T)

    th = BioheatSpectral3D(mesh, np.float64, conductivity=0.5, perfusion_rate=k_cells, fixed_tags=(3,))
    th.set_heat_source(heat_source_from(monitor, wave_solver, th))
    dt = th.stable_time_step()
    th.advance(0.0, 10.0, dt)                          # heating
    th.advance(10.0, 30.0, dt, power=(0.0, 0.0))       # cooling
    th.temperature(), th.cem43(), th.peak_temperature()

There is no CPU path.  Graph replay and sensors / monitors inside ``advance`` are not provided.
"""

from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _lib
from . import operators as ops
from .solver_base import A_RUNGE, B_RUNGE, C_RUNGE, MeshSolver3D, per_cell, rk4_steps, run_schedule, stiffness_form

# |1 - z + z^2/2 - z^3/6 + z^4/24| = 1: the stability limit of classical RK4 on the negative real axis
RK4_REAL_AXIS_LIMIT = 2.785
STAGE_FIRST, STAGE_MIDDLE, STAGE_LAST = 0, 1, 2  # csrc/bioheat.hpp


def parse_power(power):
    """The power gate ``g(t)`` of ``advance`` as a callable: ``None`` -- on (1); ``(t_on, t_off)`` -- 1 for
    ``t_on <= t < t_off``, 0 otherwise; a callable -- itself (a pulsed protocol), evaluated at the stage time."""
    if power is None:
        return lambda t: 1.0
    if callable(power):
        return lambda t: float(power(t))
    try:
        t_on, t_off = (float(x) for x in power)
    except (TypeError, ValueError):
        raise ValueError(f"power: None, (t_on, t_off) or a callable g(t), got {power!r}") from None
    if not t_on <= t_off:
        raise ValueError(f"power: t_on <= t_off expected, got ({t_on}, {t_off})")
    return lambda t: 1.0 if t_on <= t < t_off else 0.0


class InProcessGather:
    """The few host floats the ranks of one process agree on (``stable_time_step_schedule``): every rank ``put``s its values
    under a sequence number, yields, and reads all of them once its generator is resumed -- by then the lock-step driver has run
    every other rank to the same point."""

    def __init__(self, nranks):
        self.nranks, self._slots = int(nranks), {}

    def put(self, seq, rank, values):
        self._slots.setdefault(seq, {})[int(rank)] = [float(v) for v in values]

    def get(self, seq):
        got = self._slots.get(seq, {})
        if len(got) != self.nranks:
            raise _lib.FusGpuError(f"InProcessGather: {len(got)} of {self.nranks} ranks have reached reduction {seq}: drive the ranks in lock step")
        self._slots.pop(seq - 2, None)
        return np.asarray([got[r] for r in range(self.nranks)])


def _check_arguments(mesh, float_type, materials, fixed_tags):
    ft = np.dtype(float_type)
    if ft not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"float_type must be np.float32 or np.float64, got {float_type!r}")
    cells = {name: per_cell(v, mesh, name) for name, v in materials.items()}
    for name in ("conductivity", "density", "specific_heat"):
        if not np.all(np.isfinite(cells[name])) or np.any(cells[name] <= 0.0):
            raise ValueError(f"{name} must be positive and finite in every cell")
    for name in ("perfusion_rate", "blood_density", "blood_specific_heat"):
        if not np.all(np.isfinite(cells[name])) or np.any(cells[name] < 0.0):
            raise ValueError(f"{name} must be non-negative and finite in every cell")
    try:
        tags = tuple(int(t) for t in fixed_tags)
    except TypeError:
        raise ValueError(f"fixed_tags: an iterable of facet tags, got {fixed_tags!r}") from None
    return ft, cells, tags


class BioheatSpectral3D(MeshSolver3D):
    def __init__(self, mesh, float_type=np.float64, conductivity=0.5, density=1050.0, specific_heat=3600.0, perfusion_rate=0.0,
                 blood_density=1060.0, blood_specific_heat=3617.0, arterial_temperature=37.0, initial_temperature=37.0,
                 fixed_tags=(), comm=None, halo_plan=None, defer_setup_exchange=False, in_kernel_geometry="auto", affine="auto"):
        """Every material: a scalar or one value per cell in the caller's cell order (``solver_base.per_cell``).  SI units:
        ``conductivity`` W/(m K), ``density`` kg/m^3, ``specific_heat`` J/(kg K), ``perfusion_rate`` 1/s (volume of blood per
        volume of tissue and second).  ``initial_temperature``: a scalar or one value per owned dof.  ``fixed_tags``: facet tags
        (``mesh.boundary_facets``) whose dofs keep their initial value.  ``comm`` / ``halo_plan`` / ``defer_setup_exchange`` /
        ``in_kernel_geometry`` / ``affine``: as ``LinearSpectral3D``."""
        ft, cells, tags = _check_arguments(
            mesh, float_type,
            dict(conductivity=conductivity, density=density, specific_heat=specific_heat, perfusion_rate=perfusion_rate,
                 blood_density=blood_density, blood_specific_heat=blood_specific_heat), fixed_tags)
        self.Ta = float(arterial_temperature)
        self.D, G_d, self.detJ, _ = self._init_mesh(mesh, ft, comm)
        P, n, dev = self.P, self.P + 1, self.dev
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.k_cells = cells["conductivity"]
        rho_c = cells["density"] * cells["specific_heat"]
        perf = cells["perfusion_rate"] * cells["blood_density"] * cells["blood_specific_heat"]
        # the same decision on every rank: a scalar zero rate switches the term off, an array keeps it even where it is zero
        self.perfused = not (np.ndim(perfusion_rate) == 0 and float(perfusion_rate) == 0.0)
        self.cell_coeff = td((-self.k_cells).astype(ft))  # b = -K(k) T
        self._c_rho_c, self._c_perf, self._c_one = td(rho_c.astype(ft)), td(perf.astype(ft)), td(np.ones(mesh.ncells, dtype=ft))

        # ---- the stiffness operator (the G array is not kept), and the halo with one reverse closure per lumped vector ----
        self.stiff, self.G, self.affine, self.in_kernel_geometry, _ = stiffness_form(mesh, P, self.D, G_d, ft, affine, in_kernel_geometry)
        del G_d
        if self.in_kernel_geometry:
            self.x_dofs = self.G
        self.dofmap = td(mesh.dofmap)
        self.mass_cell = ops.mass_operator(n**3, ft)
        self._init_halo(halo_plan, reverse=3)

        z = lambda: torch.zeros(self.ndofs, dtype=self.tdt, device=dev)  # noqa: E731
        self.T, self.Tn, self.acc, self.b = z(), z(), z(), z()
        self.minv, self.pr, self.vol = z(), z(), z()
        self.s = None  # no heat source
        self._cem43 = torch.empty(self.nlocal, dtype=torch.float64, device=dev)  # never filled: the first step WRITES them
        self._tmax = torch.empty(self.nlocal, dtype=self.tdt, device=dev)
        self._dose_init = True
        self._fn = getattr(_lib.load(), f"fus_bioheat_stage_{_lib.suffix(self.tdt)}")
        self._limit, self._warned = None, False

        # ---- lumped vectors: M(rho C) 1, M(w_b rho_b C_b) 1, M(1) 1 and the mark of the fixed dofs -----------------------
        ones = z()
        ops.fill(1.0, ones)
        self._fix = z()
        for c, out in ((self._c_rho_c, self.minv), (self._c_perf, self.pr), (self._c_one, self.vol)):
            self.mass_cell(ones, c, out, self.detJ, self.dofmap)
        if tags:
            fd = mesh.facet_dofmap(mesh.boundary_facets(list(tags)))
            if fd.size:
                self._fix[td(np.unique(fd).astype(np.int64))] = 1.0
        self.set_temperature(initial_temperature)
        self._start_setup(defer_setup_exchange)

    def setup_schedule(self):
        """Generator: post the set-up exchange (reverse scatters of the three lumped vectors and of the fixed-dof marks), yield,
        complete it and form minv, pr.  One rank per process exhausts it in the constructor."""
        yield from self._reverse_setup((self.minv, self.pr, self.vol, self._fix))
        n = self.nlocal
        free = (self._fix[:n] == 0).to(self.tdt)
        self.mc = self.minv[:n].clone()  # M(rho C) 1 over the owned dofs
        self.minv[:n] = free / self.mc
        self.minv[n:] = 0
        self.pr[:n] *= self.minv[:n]
        self._free = free
        self._dof_volumes = self.vol[:n].to(torch.float64)  # what field_monitor.focus integrates with
        if not self.perfused:
            self.pr = None
        self._max_pr = 0.0 if self.pr is None or n == 0 else float(self.pr[:n].max().item())

    # -- state --------------------------------------------------------------------------------------------------------------
    def _owned(self, values, name):
        """A scalar or one value per owned dof (device tensor of the field type, or an array) as a device tensor [nlocal]."""
        if isinstance(values, torch.Tensor):
            if not values.is_cuda:
                raise _lib.FusGpuError(f"{name}: tensor is on {values.device}; the solver only runs on the GPU (no CPU fallback)")
            t = values.to(self.tdt)
        else:
            a = np.asarray(values, dtype=np.float64)
            if a.ndim == 0:
                return torch.full((self.nlocal,), float(a), dtype=self.tdt, device=self.dev)
            t = torch.from_numpy(np.ascontiguousarray(a.astype(self.tdt_np))).to(self.dev)
        if tuple(t.shape) != (self.nlocal,):
            raise ValueError(f"{name}: a scalar or one value per owned dof ({self.nlocal}), got shape {tuple(t.shape)}")
        return t

    def set_temperature(self, T):
        """The temperature field (deg C): a scalar or one value per owned dof.  Fixed dofs keep THIS value from here on."""
        self.T[: self.nlocal] = self._owned(T, "temperature")

    def set_heat_source(self, q):
        """``q``: the absorbed power density in W/m^3 over the owned dofs (device tensor or array; what
        ``field_monitor.heat_deposition`` returns), or ``None`` to switch the source off.  Needs the set-up exchange completed."""
        if q is None:
            self.s = None
            return
        if not hasattr(self, "mc"):
            raise _lib.FusGpuError("set_heat_source: complete the set-up exchange first (exhaust solver._setup)")
        n = self.nlocal
        qd = self._owned(q, "q").to(torch.float64)
        self.q = qd
        self.s = (self.vol[:n].to(torch.float64) * qd * self.minv[:n].to(torch.float64)).to(self.tdt).contiguous()

    def reset_dose(self):
        """Start a new dose window: the next step overwrites ``cem43`` and the peak temperature (no device work here)."""
        self._dose_init = True

    def temperature(self):
        return self.T[: self.nlocal]

    def cem43(self):
        """Cumulative equivalent minutes at 43 deg C over the owned dofs (fp64)."""
        return torch.zeros_like(self._cem43) if self._dose_init else self._cem43

    def peak_temperature(self):
        return self.T[: self.nlocal].clone() if self._dose_init else self._tmax

    def T_sol(self):
        """Owned part of the temperature field on the host."""
        return self.T[: self.nlocal].detach().cpu().numpy()

    # -- one stage ------------------------------------------------------------------------------------------------------------
    def _apply(self, x):
        """b += -K(k) x; next to a halo the interior cells overlap the forward exchange of x and the reverse exchange of b."""
        if self.halo is None:
            self.stiff(x, self.cell_coeff, self.b, self.G, self.dofmap)
        else:
            yield from self.halo.apply_schedule(x, self.cell_coeff, self.b, self.G, self.dofmap)

    def _vector_pass(self, i, dt, gate):
        last = i == 3
        kind = STAGE_LAST if last else (STAGE_FIRST if i == 0 else STAGE_MIDDLE)
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        _lib.check(
            self._fn(B_RUNGE[i] * dt, 0.0 if last else A_RUNGE[i + 1] * dt, kind, float(gate), self.Ta, float(dt), ptr(self.minv),
                     ptr(self.pr), ptr(self.s), ptr(self.b), ptr(self.T), ptr(self.Tn), ptr(self.acc), ptr(self._cem43),
                     ptr(self._tmax), int(self._dose_init), self.nlocal, self.ndofs, _lib.stream_ptr()),
            "fus_bioheat_stage",
        )
        if last:
            self._dose_init = False

    # -- the time loop ----------------------------------------------------------------------------------------------------------
    def advance(self, start_time, final_time, dt, power=None, max_steps=None):
        """Advance from ``start_time`` to ``final_time`` in steps of ``dt`` (the last one shortened); returns ``(t, steps)``.
        ``power``: see ``parse_power``.  The step is not checked against ``stable_time_step``; one warning if it exceeds the
        unscaled limit, where an earlier ``stable_time_step`` call has made that limit known (``advance`` never computes it)."""
        gate = parse_power(power)
        result = run_schedule(self.advance_schedule(start_time, final_time, dt, gate, max_steps))
        self.check_halo_health("BioheatSpectral3D.advance")
        return result

    def advance_schedule(self, start_time, final_time, dt, power=None, max_steps=None):
        """``advance`` as a generator that yields whenever this rank has posted halo exchanges (``HaloApply.schedule``); its
        return value is ``(t, steps)``.  A driver of several ranks calls ``check_halo_health()`` once they are exhausted."""
        gate = parse_power(power)
        if self._limit is not None and dt > self._limit and not self._warned:
            self._warned = True
            warnings.warn(f"BioheatSpectral3D: dt = {dt:g} s exceeds the RK4 stability limit {self._limit:g} s of this mesh "
                          "(stable_time_step(safety=1)): the temperature will grow without bound", RuntimeWarning, stacklevel=2)
        t, step = float(start_time), 0
        ops.fill(0.0, self.b)
        for t0, h in rk4_steps(t, final_time, dt, max_steps):
            for i in range(4):
                yield from self._apply(self.T if i == 0 else self.Tn)
                self._vector_pass(i, h, gate(t0 + C_RUNGE[i] * h))
            t, step = t0 + h, step + 1
        return t, step

    # -- the explicit step this mesh admits ------------------------------------------------------------------------------------
    def _gather(self, values, reduce, seq):
        """Generator: every rank's ``values`` as an array [size, len(values)]."""
        if self.halo is None:
            return np.asarray([[float(v) for v in values]])
        if reduce is not None:
            reduce.put(seq, self.comm.rank, values)
            yield "reduce"
            return reduce.get(seq)
        from .scatterer import gather_floats

        every = gather_floats(self.comm, values)
        if len(every) != self.comm.size:  # the local row alone: no bootstrap spans the ranks
            raise _lib.FusGpuError("stable_time_step: ranks driven from one process share no collective: drive "
                                   "stable_time_step_schedule(safety, reduce=InProcessGather(nranks)) in lock step")
        return every

    def stable_time_step_schedule(self, safety=0.8, reduce=None, rtol=0.01, min_iterations=16, max_iterations=200):
        """Generator form of ``stable_time_step`` (yields where ``HaloApply`` yields, and after depositing partial sums in
        ``reduce``, an ``InProcessGather`` the ranks of one process share)."""
        n, f64 = self.nlocal, torch.float64
        gen = torch.Generator().manual_seed(1234 + (self.comm.rank if self.halo is not None else 0))
        free, mc = self._free.to(f64), self.mc.to(f64)
        x = torch.zeros(self.ndofs, dtype=self.tdt, device=self.dev)
        v = (torch.rand(n, generator=gen, dtype=f64) - 0.5).to(self.dev) * free
        every = yield from self._gather([float((v * v * mc).sum().item())], reduce, 0)
        seq, vv = 1, float(every.sum())
        if not vv > 0.0:
            raise _lib.FusGpuError("stable_time_step: no free dof")
        v, v_prev, beta = v / np.sqrt(vv), torch.zeros_like(v), 0.0
        alphas, betas, lam_prev, lam = [], [], None, None
        ops.fill(0.0, self.b)
        for it in range(max_iterations):
            x[:n] = v.to(self.tdt)
            yield from self._apply(x)  # b = -K(k) x, complete over the owned dofs
            w = -self.b[:n].to(f64) * free / mc - beta * v_prev  # minv K v - beta v_prev
            ops.fill(0.0, self.b)
            every = yield from self._gather([float((w * v * mc).sum().item())], reduce, seq)
            alpha = float(every.sum())
            w -= alpha * v
            every = yield from self._gather([float((w * w * mc).sum().item())], reduce, seq + 1)
            seq, beta = seq + 2, float(np.sqrt(every.sum()))
            alphas.append(alpha)
            lam = float(np.linalg.eigvalsh(np.diag(alphas) + np.diag(betas, 1) + np.diag(betas, -1))[-1])
            if lam_prev is not None and it + 1 >= min_iterations and abs(lam - lam_prev) <= rtol * lam:
                break
            if not beta > 1e-14 * abs(lam):  # the Krylov space is exhausted: lam is exact
                break
            lam_prev = lam
            betas.append(beta)
            v_prev, v = v, w / beta
        else:
            raise _lib.FusGpuError(f"stable_time_step: the iteration did not settle to {rtol:g} in {max_iterations} applies")
        every = yield from self._gather([self._max_pr], reduce, seq)
        self.lambda_max = lam
        self._limit = RK4_REAL_AXIS_LIMIT / (self.lambda_max + float(every.max()))
        return safety * self._limit

    def stable_time_step(self, safety=0.8):
        """``safety * 2.785 / (lambda_max + max pr)``: 2.785 is the real-axis stability limit of RK4, ``lambda_max`` the largest
        eigenvalue of ``minv K(k)`` from a power iteration with the solver's own operators (on a partitioned mesh with its
        exchanges).  The quotient is taken over the whole Krylov space the iteration has spanned (the largest Ritz value of the
        Lanczos recurrence in the ``M(rho C)`` inner product: same applies, two more dot products each) -- the quotient of the
        last iterate alone settles to 1 % while still 9 % short on a 3 x 2 x 2 mesh of degree 2.  At least 16 applies, then
        until two successive values agree to 1 %; raises after 200.  Every estimate is a lower bound of ``lambda_max``."""
        dt = run_schedule(self.stable_time_step_schedule(safety))
        self.check_halo_health("BioheatSpectral3D.stable_time_step")
        return dt


def heat_source_from(monitor, wave_solver, thermal_solver=None):
    """The absorbed power density of the wave solver's last recorded window, ``field_monitor.heat_deposition(monitor,
    wave_solver)``, cast to the field type (the thermal solver's where given): the argument of ``set_heat_source``.  The two
    solvers must share the mesh partition: their ``nlocal`` must agree (and the monitor's)."""
    from .field_monitor import heat_deposition

    if monitor.nlocal != wave_solver.nlocal:
        raise ValueError(f"heat_source_from: the monitor covers {monitor.nlocal} owned dofs, the wave solver {wave_solver.nlocal}")
    if thermal_solver is not None and thermal_solver.nlocal != wave_solver.nlocal:
        raise ValueError(f"heat_source_from: the thermal solver owns {thermal_solver.nlocal} dofs, the wave solver {wave_solver.nlocal}: "
                         "build both on the same mesh and partition")
    q = heat_deposition(monitor, wave_solver)
    return q.to((thermal_solver or wave_solver).tdt)
