"""
Maps that need the spatial gradient of the pressure: the recovered gradient of a field, the particle velocity of a harmonic, the
time-averaged intensity vector and the radiation force density, all over the owned dofs and on the device.

They are compositions of one operator, the weak gradient ``C(c)`` of ``operators.gradient_operator`` (csrc/gradient_geom.hpp;
no reference counterpart), with what ``field_monitor.py`` already has:

    g = recovered_gradient(solver, field, c)        [3, nlocal]   C(c) field / M(1) 1: the lumped-mass projection of c grad(field),
                                                                  defined where the materials jump between cells
    re, im = particle_velocity(monitor, solver, k)  [3, nlocal]   V_k = i grad(P_k) / (k w rho)
    I = intensity(monitor, solver)                  [3, nlocal]   sum_k 1/2 Re(P_k conj(V_k))
    F = radiation_force(monitor, solver)            [3, nlocal]   sum_k 2 alpha_k I_k / c

``P_k = (2 / N)(hre + i him)`` is the monitor's own convention, ``p_k(t) = Re(P_k e^{i k w t})`` (``FieldMonitor.harmonic_phase``),
and ``w = 2 pi monitor.frequency``.  Every function has a ``*_schedule`` generator for drivers that advance several ranks from one
process (a ``yield`` after each posted halo exchange, as ``field_monitor.lumped_mass_schedule``).  ``|I|`` and ``|F|`` go through
``field_monitor.focus``.
"""

from __future__ import annotations

import numpy as np

from .field_monitor import dof_volumes_schedule, lumped_mass_schedule


def _gradient_operator(solver):
    """The solver's gradient operator, built on demand from the mesh vertices and kept on the solver (as ``_dof_volumes``): it does
    not depend on which stiffness form the solver chose (affine, G stream, in-kernel geometry)."""
    op = getattr(solver, "_gradient_op", None)
    if op is None:
        from . import operators as ops
        from .gll import tabulate_1d
        from .solver_base import vertex_geometry

        D = tabulate_1d(solver.P, solver.tdt_np)[2]
        op = ops.gradient_operator(solver.P, D.flatten(), solver.tdt_np, geometry=vertex_geometry(solver.mesh, solver.P, solver.dev))
        solver._gradient_op = op
    return op


def _check_field(solver, field, name):
    import torch

    if not isinstance(field, torch.Tensor):
        raise TypeError(f"{name}: expected a device tensor, got {type(field).__name__}")
    if field.dim() != 1 or field.numel() not in (solver.nlocal, solver.ndofs):
        raise ValueError(f"{name}: a vector over the owned dofs ({solver.nlocal}) or over all dofs ({solver.ndofs}), got {tuple(field.shape)}")
    if not field.is_cuda:
        from ._lib import FusGpuError

        raise FusGpuError(f"{name}: tensor is on {field.device}; the maps are formed on the GPU (no CPU fallback)")


def _cell_constants(solver, cell_constants):
    c = np.ones(solver.mesh.ncells) if cell_constants is None else np.asarray(cell_constants, dtype=np.float64)
    if c.shape != (solver.mesh.ncells,):
        raise ValueError(f"cell_constants: one value per cell ({solver.mesh.ncells}), got shape {c.shape}")
    return c


def recovered_gradient_schedule(solver, field, cell_constants=None):
    """Generator form of ``recovered_gradient``."""
    import torch

    _check_field(solver, field, "field")
    c = _cell_constants(solver, cell_constants)
    op = _gradient_operator(solver)
    cc = torch.from_numpy(np.ascontiguousarray(c.astype(solver.tdt_np))).to(solver.dev)
    x = torch.zeros(solver.ndofs, dtype=solver.tdt, device=solver.dev)
    m = min(field.numel(), solver.ndofs)
    x[:m] = field[:m].to(solver.tdt)
    if solver.halo is not None:  # the ghosts of the field: whatever the caller's tensor holds there is not trusted
        wk = solver.halo.fwd.begin(x)
        yield "forward"
        solver.halo.fwd.end(x, wk)
    y3 = torch.zeros((3, solver.ndofs), dtype=solver.tdt, device=solver.dev)
    op(x, cc, y3, solver.dofmap)
    if solver.halo is not None:  # contributions of this rank's cells to dofs other ranks own, one component after the other
        for d in range(3):
            wk = solver.halo.rev.begin(y3[d])
            yield "reverse"
            solver.halo.rev.end(y3[d], wk)
    vol = yield from dof_volumes_schedule(solver)
    return y3[:, : solver.nlocal].to(torch.float64) / vol


def recovered_gradient(solver, field, cell_constants=None):
    """``C(c) field / M(1) 1`` over the owned dofs, ``[3, nlocal]`` fp64: the lumped-mass projection of ``c grad(field)`` (default
    ``c = 1``).  ``field``: a device tensor over the owned dofs or over all dofs of the solver's mesh (the ghost entries are
    exchanged here).  ``cell_constants``: one value per cell in the mesh's cell order (host array)."""
    from .solver_base import run_schedule

    return run_schedule(recovered_gradient_schedule(solver, field, cell_constants))


def _inverse_density(solver):
    rho = getattr(solver, "rho_cells", None)
    if rho is None:
        raise ValueError("the solver keeps no per-cell rho_cells (LinearSpectral3D and WesterveltSpectral3D do)")
    return 1.0 / np.asarray(rho, dtype=np.float64)


def _harmonic_number(k, omega):
    if int(k) != k or int(k) < 1:
        raise ValueError(f"harmonic number k must be an integer >= 1, got {k!r}")
    if not float(omega) > 0.0:
        raise ValueError(f"omega must be > 0, got {omega!r}")
    return int(k), float(omega)


def _monitor_harmonic(monitor, k):
    """``(Re P_k, Im P_k, w)`` of the monitor's k-th harmonic, ``P_k = (2 / N)(hre + i him)``."""
    if getattr(monitor, "omega", None) is None:
        raise ValueError("the monitor accumulates no harmonics (harmonics=(), frequency=None)")
    hre, him = monitor._harmonic(k)
    s = 2.0 / monitor.nacc
    return hre * s, him * s, float(monitor.omega)


def particle_velocity_schedule(monitor, solver, k):
    """Generator form of ``particle_velocity``."""
    rinv = _inverse_density(solver)
    re, im, omega = _monitor_harmonic(monitor, k)
    k, omega = _harmonic_number(k, omega)
    g_re = yield from recovered_gradient_schedule(solver, re, rinv)
    g_im = yield from recovered_gradient_schedule(solver, im, rinv)
    return -g_im / (k * omega), g_re / (k * omega)  # i (g_re + i g_im) / (k w)


def particle_velocity(monitor, solver, k):
    """``(re, im)``, each ``[3, nlocal]`` fp64, of the particle velocity amplitude of the monitor's k-th harmonic:
    ``V_k = i grad(P_k) / (k w rho)`` (from ``rho dv/dt = -grad p`` with ``e^{i k w t}``), ``1 / rho`` per cell as the gradient
    operator's cell constant (``solver.rho_cells``; of a solver with a nodal medium the per-cell mean of its nodal rho: exact nodal
    rho here is out of scope)."""
    from .solver_base import run_schedule

    return run_schedule(particle_velocity_schedule(monitor, solver, k))


def intensity_of_schedule(solver, k, omega, re, im):
    """Generator form of ``intensity_of``."""
    k, omega = _harmonic_number(k, omega)
    rinv = _inverse_density(solver)
    _check_field(solver, re, "re")
    _check_field(solver, im, "im")
    import torch

    g_re = yield from recovered_gradient_schedule(solver, re, rinv)
    g_im = yield from recovered_gradient_schedule(solver, im, rinv)
    n = solver.nlocal
    return (im[:n].to(torch.float64) * g_re - re[:n].to(torch.float64) * g_im) / (2.0 * k * omega)


def intensity_of(solver, k, omega, re, im):
    """The intensity of one harmonic given as explicit device tensors ``re = Re P_k``, ``im = Im P_k`` (over the owned or all dofs):
    ``1/2 Re(P_k conj(V_k)) = (Im P_k g(Re P_k) - Re P_k g(Im P_k)) / (2 k w)``, ``g`` the recovered gradient with cell constant
    ``1 / rho``.  ``[3, nlocal]`` fp64."""
    from .solver_base import run_schedule

    return run_schedule(intensity_of_schedule(solver, k, omega, re, im))


def _harmonics_of(monitor, harmonics):
    kept = tuple(getattr(monitor, "harmonics", ()))
    hs = kept if harmonics is None else tuple(harmonics)
    if not hs:
        raise ValueError("intensity: the monitor keeps no harmonics")
    for k in hs:
        if k not in kept:
            raise ValueError(f"harmonic {k} is not accumulated (harmonics={kept})")
    return hs


def intensity_schedule(monitor, solver, harmonics=None):
    """Generator form of ``intensity``."""
    hs = _harmonics_of(monitor, harmonics)
    _inverse_density(solver)
    total = None
    for k in hs:
        re, im, omega = _monitor_harmonic(monitor, k)
        part = yield from intensity_of_schedule(solver, k, omega, re, im)
        total = part if total is None else total + part
    return total


def intensity(monitor, solver, harmonics=None):
    """The time-averaged intensity vector ``I = sum_k 1/2 Re(P_k conj(V_k))`` over ``harmonics`` (default: every harmonic the
    monitor keeps), ``[3, nlocal]`` fp64."""
    from .solver_base import run_schedule

    return run_schedule(intensity_schedule(monitor, solver, harmonics))


def radiation_force_schedule(monitor, solver):
    """Generator form of ``radiation_force``."""
    for name in ("delta_cells", "rho_cells", "c_cells"):
        if not hasattr(solver, name):
            raise ValueError(f"radiation_force: the solver keeps no per-cell {name} (a WesterveltSpectral3D does)")
    hs = _harmonics_of(monitor, None)
    delta, c = np.asarray(solver.delta_cells, dtype=np.float64), np.asarray(solver.c_cells, dtype=np.float64)
    vol = yield from dof_volumes_schedule(solver)
    total = None
    for k in hs:
        re, im, omega = _monitor_harmonic(monitor, k)
        part = yield from intensity_of_schedule(solver, k, omega, re, im)
        two_alpha_over_c = delta * (k * omega) ** 2 / c**4  # 2 alpha_k / c, alpha_k = delta (k w)^2 / (2 c^3)
        mk = yield from lumped_mass_schedule(solver, two_alpha_over_c)
        part = part * (mk / vol)
        total = part if total is None else total + part
    return total


def radiation_force(monitor, solver):
    """The radiation force density ``F = sum_k (M(2 alpha_k / c) 1 / M(1) 1) I_k`` with ``alpha_k = delta (k w)^2 / (2 c^3)`` per
    cell -- the ``delta``, ``rho``, ``c`` per cell that ``field_monitor.heat_deposition`` reads.  ``[3, nlocal]`` fp64."""
    from .solver_base import run_schedule

    return run_schedule(radiation_force_schedule(monitor, solver))


def magnitude(vec3):
    """``|v|`` of a ``[3, n]`` map, for ``field_monitor.focus``."""
    return (vec3 * vec3).sum(dim=0).sqrt()
