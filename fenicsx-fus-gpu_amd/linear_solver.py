"""
Linear acoustic wave solver (explicit RK4 on u' = v, M v' = -K u + boundary terms) on the
synthetic box mesh, driven entirely by this package's operators and scatterers -- the
"demo_linear_box" caller of the hot path (BASELINE config 3).

Semantics follow the reference drivers:
  set-up        cuda/demo_linear_box.py:245-345 (geometry factors, source facets x = 0,
                absorbing facets x = L, material coefficients), :421-428 (lumped mass
                m = M(1/(rho c^2)) 1, scatter_rev)
  time step     cuda/demo_linear_box.py:115-122 (dt = CFL h / (c P^2), snapped to an integer
                number of steps per period; final time L/c + 2/f)
  RK4 stage     cuda/demo_linear_box.py:487-566; source window / g evaluated at the STAGE
                time tn as fenicsx/demo_linear_box.py:187-199,270, numba-cpu/demo_linear_box.py:345-358
                and cpp/common/Linear.hpp:179-187,317 do (the CUDA demos use t -- SURVEY 3.4 quirks;
                ``source_time="t"`` reproduces them)
The class shape mirrors cpp/common/Linear.hpp:52-348 (LinearSpectral3D: init / rk4 / u_sol).

Two stage implementations with identical results up to round-off:
  fused=False   the reference's exact launch sequence (5 copy, 4 axpy, 2 fill, 1 divide, 3 operator
                applies, 3 scatters per stage), through the reference-compatible call surface;
  fused=True    one fused vector kernel per stage (csrc/rk4.hpp), ku doubling as v_n, the source
                term through scaled facet constants instead of a full-vector fill, 1/m precomputed,
                halo exchange overlapped with interior cells.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import operators as ops
from .solver_base import A_RUNGE, B_RUNGE, SpectralSolver3D, per_cell, stiffness_form


def time_step_parameters(mesh, P, speed_of_sound, source_frequency, domain_length, CFL=0.65):
    """cuda/demo_linear_box.py:115-122.  ``mesh_size`` = smallest cell diameter (dolfinx
    ``cpp.mesh.h``: largest vertex-vertex distance of a cell), min over ranks by the caller."""
    xg = mesh.x_g.astype(np.float64)[mesh.x_dofs]  # [nc, 8, 3]
    d = np.linalg.norm(xg[:, :, None, :] - xg[:, None, :, :], axis=-1).reshape(mesh.ncells, -1).max(axis=1)
    return float(d.min())


def snap_time_step(mesh_size, P, speed_of_sound, source_frequency, domain_length, CFL=0.65):
    period = 1.0 / source_frequency
    dt = CFL * mesh_size / (speed_of_sound * P**2)
    step_per_period = int(period / dt) + 1
    dt = period / step_per_period
    final_time = domain_length / speed_of_sound + 2.0 / source_frequency
    return dt, final_time, int((final_time - 0.0) / dt) + 1


class LinearSpectral3D(SpectralSolver3D):
    def __init__(self, mesh, float_type=np.float64, speed_of_sound=1500.0, density=1000.0,
                 source_frequency=0.5e6, source_amplitude=60000.0, comm=None, fused=True,
                 source_time="tn", overlap=True, halo_kernels=None, affine="auto", in_kernel_geometry="auto",
                 halo_plan=None, defer_setup_exchange=False, reference_speed_of_sound=None, keep_G=False, source=None,
                 sponge=None, point_source=None, point_claim=None, relaxation=None, nodal_medium=None):
        """``speed_of_sound`` / ``density``: scalars, or one value per cell (heterogeneous medium: the DG0 material arrays of
        the reference's drivers, in the caller's cell order).  ``reference_speed_of_sound``: the c of the source term
        ``p0 w0 / c cos(w0 t)`` (cuda/demo_linear_box.py:515-530 uses the scalar of its homogeneous medium); default: the
        scalar given, or the mean over the cells of the source facets.
        ``in_kernel_geometry``: ``"auto"`` (default) -- on non-affine cells of degree >= 3 the stiffness apply forms G in the kernel
        from the 8 vertices of each cell (the reference's geometry is P1 everywhere, cuda/demo_nonlinear_bowl.py:317): -18 % per
        step and no 6 n^3-value-per-cell G array at config 3; ``False`` keeps the reference's G stream
        (numba-cpu/precompute.py:115-163), ``True`` forces the kernel form for any degree.  ``keep_G``: keep the G array on the
        device although the apply does not read it (``solver.G_array``).  ``source``: a ``sources.SourceArray`` (phased array:
        per-element amplitude, phase and delay, optionally a burst) in place of the one scalar waveform of ``source_value``;
        bound to this rank's source facets here (``self.source``), ``None`` keeps every launch as it is.  ``sponge``: a
        ``sponge.SpongeLayer`` (absorbing layer: b -= 2 sigma m v_n + sigma^2 m u_n over its owned dofs, one sparse launch per stage
        after the facet terms); ``None`` keeps every launch as it is.  ``point_source``: a ``sources.PointSources`` (monopoles inside
        the volume: b[dofmap[c][ijk]] += g_p(t) Lx[i] Ly[j] Lz[k], one launch per stage after the facet terms, at the stage's source
        time); it coexists with ``source``, the scalar source and ``sponge``; ``source_amplitude=0.0`` silences the facet source for a
        receive run (the virtual source of a time-reversal run, receivers.py).  ``None`` keeps every launch as it is.
        ``point_claim``: this rank's row of ``sources.claim_points`` when several ranks are driven from one process (handed in like
        ``halo_plan``); ranks in different processes agree through one gather.  ``relaxation``: a
        ``relaxation.RelaxationAbsorption`` (power-law absorption: memory variables xi' = kappa v - xi / tau per mechanism, the stiffness
        apply acts on u_n + sum xi, one streaming launch per stage); ``speed_of_sound`` is then the EQUILIBRIUM (low-frequency) speed,
        the phase speed rises with frequency (``RelaxationAbsorption.phase_speed``).  ``None`` keeps every launch as it is.
        ``nodal_medium``: a ``nodal_medium.NodalMedium`` -- c and rho at the DOFS (n times finer per axis than one value per cell, on
        the same mesh) in place of ``speed_of_sound`` / ``density``, which must then be left scalar (arrays raise).  The stiffness
        apply takes 1/rho inside its contraction (the nodal kernel with the geometry formed in the kernel, at every degree and on
        affine boxes too; ``in_kernel_geometry=False``: the general kernel on a G array scaled once; ``affine=True`` raises); the
        lumped mass is ``(M(1) 1, reverse-scattered) * 1/(rho c^2)``.  The facet terms keep ONE coefficient per facet, the mean of
        the nodal coefficient (1/rho on the source facets, 1/(rho c) on the absorbing ones) over that facet's dofs: exact where the
        medium is constant on a boundary facet, and the source and absorbing faces are expected to lie in the coupling medium.
        ``rho_nodal`` / ``c_nodal`` hold the fields (host, float64, local dofs); ``rho_cells`` / ``c_cells`` the per-cell MEANS of the
        nodal values, which is what ``intensity.py``, ``field_monitor.heat_deposition`` and per-cell relaxation weights then see.
        ``reference_speed_of_sound`` defaults to the mean of c over the dofs of the source facets.  ``None`` keeps every launch as it
        is."""
        self.nodal_medium, self.c_nodal, self.rho_nodal = nodal_medium, None, None
        if nodal_medium is not None:
            if np.ndim(speed_of_sound) != 0 or np.ndim(density) != 0:
                raise ValueError("nodal_medium= together with speed_of_sound= / density= arrays: the nodal medium is the medium, "
                                 "leave the two per-cell arguments scalar")
            from .nodal_medium import cell_means, facet_means

            self.c_nodal, self.rho_nodal = nodal_medium.evaluate(mesh)
            speed_of_sound, density = cell_means(self.c_nodal, mesh.dofmap), cell_means(self.rho_nodal, mesh.dofmap)
            c_cells, rho_cells = speed_of_sound, density  # already in the mesh's cell order
        else:
            c_cells, rho_cells = per_cell(speed_of_sound, mesh, "speed_of_sound"), per_cell(density, mesh, "density")
        bd1, bd2, D, G_d, detJ_d, (dF1_d, dF2_d) = self._init_common(mesh, float_type, comm, fused, source_time)
        self._init_relaxation(relaxation)
        self.c0, self.rho0 = float(c_cells.mean()), float(rho_cells.mean())
        self.rho_cells, self.c_cells = rho_cells, c_cells  # per cell, the mesh's cell order (intensity.py)
        self.f0, self.p0 = float(source_frequency), float(source_amplitude)
        self.w0 = 2.0 * np.pi * self.f0
        self._init_terms(sponge, point_source, point_claim)
        P, n, dev, ft = self.P, self.P + 1, self.dev, self.tdt_np
        self.D = D
        rho, c = rho_cells.astype(ft), c_cells.astype(ft)
        if reference_speed_of_sound is not None:
            self.c0 = float(reference_speed_of_sound)
        elif nodal_medium is not None:
            if bd1.shape[0]:
                self.c0 = float(self.c_nodal[mesh.facet_dofmap(bd1)].mean())
        elif np.ndim(speed_of_sound) == 0:
            self.c0 = float(speed_of_sound)
        elif bd1.shape[0]:
            self.c0 = float(c_cells[bd1[:, 0]].mean())
        td = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        fd1, fd2 = mesh.facet_dofmap(bd1), mesh.facet_dofmap(bd2)
        if nodal_medium is None:
            self.cell_coeff1 = td(1.0 / rho / c / c)  # :336
            self.cell_coeff2 = td(-1.0 / rho)  # :337
            self.facet_coeff1 = td((1.0 / rho[bd1[:, 0]]).astype(ft))  # :339-341
            self.facet_coeff2 = td((-1.0 / rho[bd2[:, 0]] / c[bd2[:, 0]]).astype(ft))  # :343-345
            kappa = None
        else:  # the medium sits in the operators' nodal factors: unit cell constants (-1 for the stiffness), one mean per facet
            self.cell_coeff1 = td(np.ones(mesh.ncells, dtype=ft))
            self.cell_coeff2 = td(np.full(mesh.ncells, -1.0, dtype=ft))
            self.facet_coeff1 = td(facet_means(1.0 / self.rho_nodal, fd1).astype(ft))
            self.facet_coeff2 = td((-facet_means(1.0 / (self.rho_nodal * self.c_nodal), fd2)).astype(ft))
            kappa = (1.0 / self.rho_nodal).astype(ft)
            self._mass_factor = td((1.0 / (self.rho_nodal * self.c_nodal**2)).astype(ft))  # the diagonal of the lumped mass
        self.G, self.detJ, self.dofmap = G_d, detJ_d, td(mesh.dofmap)
        self.detJ_f1, self.detJ_f2 = dF1_d, dF2_d
        self.fdm1, self.fdm2 = td(fd1), td(fd2)
        # the fused stage's facet sets: M_f1(g c1) 1 with g = source_value(t) -- or, with a phased-array source (sources.py), through
        # fus_facet_source_array_* with g = p0 w0 / c0 per element -- and M_f2(c2) v_n
        self._init_source(source, bd1, self.p0 * self.w0 / self.c0, (self.facet_coeff1, None, self.detJ_f1, self.fdm1))
        self._absorbing_set = (self.facet_coeff2, self.detJ_f2, self.fdm2)

        # ---- operators and halo ---------------------------------------------------------------------
        self.stiff, self.G, self.affine, self.in_kernel_geometry, self.G_array = stiffness_form(
            mesh, P, D, G_d, ft, affine, in_kernel_geometry, keep_G, nodal=kappa)
        del G_d
        if self.in_kernel_geometry:
            self.x_dofs = self.G
        self.mass_cell = ops.mass_operator(n**3, ft)
        self.mass_facet = ops.mass_operator(n * n, ft)
        self.axpy = ops.axpy(self.ndofs)
        self.fwd_v, = self._init_halo(halo_plan, forward=1, overlap=overlap, kernels=halo_kernels)
        # the facet mass applies of a stage are ``boundary_terms`` of HaloApply: in its concurrent schedule they run on the
        # communicator's stream WHILE the interior stiffness launch adds into the same b with float atomics (interior cells
        # on the x = 0 / x = L faces touch exactly the facet dofs).  The atomic-free gather kernel's plain load + store would
        # lose those adds: next to a halo the facet operator is the float-atomic twin.
        self._mass_facet_stage = self.mass_facet if self.halo is None else self.halo.concurrent_safe(self.mass_facet)

        z = lambda: torch.zeros(self.ndofs, dtype=self.tdt, device=dev)  # noqa: E731
        self.u, self.v, self.u0, self.v0 = z(), z(), z(), z()
        self.un, self.vn, self.ku, self.kv = z(), z(), z(), z()
        self.u_n, self.v_n, self.g, self.b, self.m = z(), z(), z(), z(), z()

        # ---- lumped mass: m = M(1/(rho c^2)) 1, reverse-scattered (:421-428); a nodal medium: M(1) 1, its factor after the exchange
        ops.fill(1.0, self.g)
        # the default operator (atomic-free, bitwise reproducible): nothing else adds into m while it runs -- the reverse scatter
        # of m follows it in stream order
        self.mass_cell(self.g, self.cell_coeff1, self.m, self.detJ, self.dofmap)
        self.minv = z()
        self._start_setup(defer_setup_exchange)
        # g stays 1 for the fused path (source enters through scaled facet constants)

    def setup_schedule(self):
        """Generator: post the set-up exchange (reverse scatter of the lumped mass), yield, complete it and
        form 1/m.  One rank per process exhausts it in the constructor."""
        yield from self._reverse_setup([self.m])
        if self.nodal_medium is not None:  # m = (M(1) 1, assembled) * 1/(rho c^2): one pointwise product over the owned dofs
            self.m[: self.nlocal].mul_(self._mass_factor[: self.nlocal])
        ops.fill(1.0, self.minv)
        ops.pointwise_divide(self.minv, self.m, self.minv)  # owned entries are what the fused kernel reads
        self._bind_terms(self.m)  # m is complete only now
        yield from self._bind_relaxation()

    def source_value(self, t):
        """Window x p0 w0 / c0 x cos(w0 t) (cuda/demo_linear_box.py:515-530)."""
        T, alpha = 1.0 / self.f0, 4.0
        window = 0.5 * (1.0 - np.cos(self.f0 * np.pi * t / alpha)) if t < T * alpha else 1.0
        return window * self.p0 * self.w0 / self.c0 * np.cos(self.w0 * t)

    def _source_scalars(self, t):
        return (self.source_value(t), 0.0)

    def _cell_terms(self, u_n, v_n, facets):
        """b += K(c2) u_n, then ``facets()``; next to a halo the interior cells overlap the exchange of u_n and v_n."""
        if self.halo is None:
            self.stiff(u_n, self.cell_coeff2, self.b, self.G, self.dofmap)
            facets()
        else:
            yield from self.halo.apply_schedule(u_n, self.cell_coeff2, self.b, self.G, self.dofmap,
                                                extra_forward=[(self.fwd_v, v_n)], boundary_terms=facets)

    def _stiffness_operator(self):
        """K(-1/rho) as the stages apply it (``solver_base._stiffness_of``: the energy record and ``stable_time_step``)."""
        return self.stiff, self.cell_coeff2, self.G, self.dofmap

    def _energy_mass(self):
        """The lumped mass the stage divides by."""
        return self.m

    # -- reference launch sequence ----------------------------------------------------------------
    def _stage_reference(self, i, t, dt):
        copy, fill, axpy = ops.copy, ops.fill, self.axpy
        copy(self.u0, self.un)
        copy(self.v0, self.vn)
        axpy(A_RUNGE[i] * dt, self.ku, self.un)
        axpy(A_RUNGE[i] * dt, self.kv, self.vn)
        copy(self.vn, self.ku)  # f0
        ts = self._stage_time(t, i, dt)
        if self.source is None:  # the reference's own launches: g filled into a vector, then its facet mass apply
            fill(self.source_value(ts), self.g)
            source_facets = lambda: self._mass_facet_stage(self.g, self.facet_coeff1, self.b, self.detJ_f1, self.fdm1)  # noqa: E731
        else:  # the array's source facets alone (no set B) replace both
            source_facets = lambda: self._facet_source.launch(self.b, None, t=ts)  # noqa: E731
        copy(self.un, self.u_n)
        copy(self.vn, self.v_n)
        fill(0.0, self.b)

        def facets():
            source_facets()
            self._mass_facet_stage(self.v_n, self.facet_coeff2, self.b, self.detJ_f2, self.fdm2)
            self._extra_terms(self.u_n, self.v_n, ts)

        yield from self._cell_terms(self._stiffness_input(self.u_n), self.v_n, facets)
        ops.pointwise_divide(self.b, self.m, self.kv)
        axpy(B_RUNGE[i] * dt, self.ku, self.u)
        axpy(B_RUNGE[i] * dt, self.kv, self.v)
        self._relax_reference(i, dt)

    # -- fused: one vector kernel per stage (csrc/rk4.hpp) -------------------------------------------
    def _vector_pass(self, bw, aw, new_step):
        fn = getattr(_lib.load(), f"fus_rk4_stage_{_lib.suffix(self.tdt)}")
        _lib.check(
            fn(float(bw), float(aw), int(new_step), self.minv.data_ptr(), self.b.data_ptr(), self.u.data_ptr(),
               self.v.data_ptr(), self.u0.data_ptr(), self.v0.data_ptr(), self.ku.data_ptr(), self.un.data_ptr(),
               self.nlocal, self.ndofs, _lib.stream_ptr()),
            "fus_rk4_stage",
        )
