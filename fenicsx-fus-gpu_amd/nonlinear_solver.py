"""
Westervelt (nonlinear) acoustic wave solver on the synthetic mesh -- the caller of BASELINE
config 5 (cuda/demo_nonlinear_bowl.py / demo_nonlinear_box.py): per RK4 stage two stiffness
applies (u_n with -1/rho, v_n with -delta/(rho c^2)), a solution-dependent lumped mass
m = m0 + M(-2 beta/(rho^2 c^4)) u_n, the quadratic term M(2 beta/(rho^2 c^4)) v_n^2 and the
source / absorbing boundary-facet terms (cuda/demo_nonlinear_bowl.py:357-374, 458-475, 540-650).

The reference's transducer mesh (H131/mesh.xdmf) is not in its repository; the geometry here is
the synthetic box, optionally warped into non-affine trilinear cells (``BoxMesh(warp=...)``), with
the source on x = 0 and the absorbing condition on x = L as in cuda/demo_nonlinear_box.py.
The stage follows the reference's launch sequence through the reference-compatible operators.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import operators as ops
from .solver_base import A_RUNGE, B_RUNGE, IN_KERNEL_GEOMETRY_FROM_DEGREE, SpectralSolver3D, per_cell, vertex_geometry


def compute_diffusivity_of_sound(frequency, speed, attenuationdB):
    """cuda/utils.py:157-162."""
    attenuationNp = attenuationdB / 20 * np.log(10)
    return 2 * attenuationNp * speed**3 / frequency / frequency


# The fused stage's cell pass with a nodal medium where ``nodal_cell_pass="auto"``: the one-pass kernel
# (westervelt_cell_geom_nodal_kernel) or two launches of the nodal stiffness kernel (tools/time_westervelt_nodal.py decides)
NODAL_CELL_PASS_DEFAULT = "fused"


class WesterveltSpectral3D(SpectralSolver3D):
    def __init__(self, mesh, float_type=np.float64, speed_of_sound=1480.0, density=1000.0,
                 source_frequency=1.1e6, source_amplitude=None, nonlinear_coefficient=3.5,
                 attenuation_coefficient_dB=0.2, comm=None, source_time="tn", overlap=True, fused=False,
                 in_kernel_geometry="auto", uniform_ratio="auto", halo_plan=None, defer_setup_exchange=False,
                 reference_speed_of_sound=None, reference_density=None, keep_G=False, source=None, sponge=None,
                 point_source=None, point_claim=None, relaxation=None, nodal_medium=None, nodal_cell_pass="auto", shock_capture=None):
        """``speed_of_sound``, ``density``, ``nonlinear_coefficient``, ``attenuation_coefficient_dB``: scalars, or one value per
        cell in the caller's cell order (the DG0 material arrays of cuda/demo_nonlinear_bowl.py:166-178 -- water / skull / ...).
        ``reference_speed_of_sound`` / ``reference_density``: the scalars of the source term and of the default source amplitude
        (the reference uses those of the coupling medium); default: the scalars given, or the means over the source-facet cells.
        ``uniform_ratio``: ``True`` opts into the single-gather cell pass where c4 / c3 = delta / c^2 is uniform (any homogeneous
        medium); the default is the two-gather pass for every medium (faster since round 5, and what a heterogeneous medium needs anyway).
        ``in_kernel_geometry``: ``"auto"`` (default) -- the fused stage of degree >= 3 forms G in the cell kernel from the 8
        vertices of each (trilinear) cell and the G array is dropped unless ``keep_G``; ``False``: the reference's G stream;
        the reference launch sequence (``fused=False``) always reads G.  ``source``: a ``sources.SourceArray`` (phased array) in
        place of the one waveform of ``source_values``, as ``LinearSpectral3D``; ``None`` keeps every launch as it is.  ``sponge``: a
        ``sponge.SpongeLayer`` (absorbing layer), as ``LinearSpectral3D``, with the steady lumped mass m0 in its coefficients -- the
        effective damping is then 2 sigma m0 / (m0 + w2 u_n), by definition; ``None`` keeps every launch as it is.  ``point_source`` /
        ``point_claim``: a ``sources.PointSources`` (monopoles inside the volume), as ``LinearSpectral3D``; it coexists with ``source``,
        the scalar source and ``sponge``, and ``source_amplitude=0.0`` silences the facet source for a receive run; ``None`` keeps
        every launch as it is.  ``relaxation``: a ``relaxation.RelaxationAbsorption`` (power-law absorption), as ``LinearSpectral3D``:
        K(c3) acts on u_n + sum xi, K(c4) on v_n as before, and the thermoviscous ``attenuation_coefficient_dB`` adds its f^2 part
        (``relaxation.fit_power_law`` fits both together); ``speed_of_sound`` is then the EQUILIBRIUM (low-frequency) speed.  The
        single-gather form is out of scope: with ``uniform_ratio=True`` a ``ValueError``.  ``None`` keeps every launch as it is.
        ``nodal_medium``: a ``nodal_medium.NodalMedium`` -- c, rho, beta and alpha at the DOFS in place of the four per-cell
        arguments, which must then be left scalar (a field the medium leaves ``None`` takes the scalar).  With
        ``delta = compute_diffusivity_of_sound(w0, c, alpha)`` at the dofs the cell pass is
        ``b -= sum_q B_q^T G_q (1/rho grad u_n + delta/(rho c^2) grad v_n)``, the coefficients inside the contractions
        (csrc/westervelt_geom_nodal.hpp; G formed in the kernel at every degree, ``in_kernel_geometry=False`` and
        ``uniform_ratio=True`` raise), and the three diagonals are ONE unit-coefficient mass apply times nodal factors:
        ``m0 = M(1)1 / (rho c^2)`` + the facet term, ``w2 = M(1)1 (-2 beta / (rho^2 c^4))``, ``w5 = -w2``.  The facet terms keep one
        coefficient per facet, the mean over the facet's dofs of the nodal expression.  ``c_nodal`` ... ``att_nodal`` hold the fields,
        ``c_cells`` / ``rho_cells`` / ``delta_cells`` the per-cell means, ``c0`` / ``rho0`` default to the means over the source facets'
        dofs.  ``fused=False`` runs two launches of the nodal stiffness operator and pointwise products with ``w2`` / ``w5`` (no
        reverse scatter of m).  ``nodal_cell_pass``: ``"fused"`` (the one-pass kernel), ``"two-launch"`` (the fused stage takes the
        two launches of the nodal stiffness operator instead) or ``"auto"``: ``NODAL_CELL_PASS_DEFAULT``.
        ``shock_capture``: a ``shock_capture.ShockCapture`` -- after a step (every ``every``-th) one sensor launch on the new field adds
        artificial diffusivity to ``delta`` of the cells where the wave steepens, by rewriting ``self.cc4`` in place (``cc4_base`` keeps
        the physical constants); the cell pass and the reference launch sequence read ``self.cc4`` as before, the facet coefficients
        keep the physical ``delta``, and ``stable_time_step`` counts the largest diffusivity a cell can get.  On a partitioned mesh a
        due launch posts one forward exchange of the field first.  ``uniform_ratio=True`` (the single-gather form needs ONE ratio
        delta / c^2) and ``nodal_medium=`` (there ``cc4`` is a unit multiplier of a nodal coefficient: out of scope) raise
        ``ValueError``.  ``None`` leaves every launch as it is."""
        if shock_capture is not None and uniform_ratio is True:
            raise ValueError("shock_capture= with uniform_ratio=True: the single-gather form needs one ratio delta / c^2 for the whole "
                             "medium, the artificial diffusivity differs from cell to cell")
        if shock_capture is not None and nodal_medium is not None:
            raise ValueError("shock_capture= with nodal_medium=: the nodal cell pass takes delta / (rho c^2) at the dofs and cc4 is a "
                             "unit multiplier there; shock capturing for nodal media is out of scope (DESIGN 7)")
        self.nodal_medium = nodal_medium
        if nodal_medium is not None:
            given = {"speed_of_sound": speed_of_sound, "density": density, "nonlinear_coefficient": nonlinear_coefficient,
                     "attenuation_coefficient_dB": attenuation_coefficient_dB}
            arrays = [k for k, val in given.items() if np.ndim(val) != 0]
            if arrays:
                raise ValueError(f"nodal_medium= together with array(s) for {', '.join(arrays)}: the nodal medium is the medium, leave "
                                 "the per-cell arguments scalar")
            if uniform_ratio is True:
                raise ValueError("nodal_medium= with uniform_ratio=True: the single-gather form needs one ratio delta / c^2 for the "
                                 "whole medium")
            if in_kernel_geometry is False:
                raise ValueError("nodal_medium= with in_kernel_geometry=False: the nodal cell pass forms G in the kernel; two G arrays "
                                 "scaled by the two coefficients (12 n^3 values per cell) are not worth carrying")
            if nodal_cell_pass not in ("auto", "fused", "two-launch"):
                raise ValueError(f"nodal_cell_pass={nodal_cell_pass!r}: 'auto', 'fused' or 'two-launch'")
            from .nodal_medium import cell_means, facet_means

            self.c_nodal, self.rho_nodal, self.beta_nodal, self.att_nodal = nodal_medium.evaluate_westervelt(
                mesh, nonlinear_coefficient, attenuation_coefficient_dB)
            self.delta_nodal = compute_diffusivity_of_sound(2 * np.pi * float(source_frequency), self.c_nodal, self.att_nodal)
            speed_of_sound, density = cell_means(self.c_nodal, mesh.dofmap), cell_means(self.rho_nodal, mesh.dofmap)
            nonlinear_coefficient = cell_means(self.beta_nodal, mesh.dofmap)
            attenuation_coefficient_dB = cell_means(self.att_nodal, mesh.dofmap)
        if relaxation is not None and uniform_ratio is True:
            raise ValueError("WesterveltSpectral3D: relaxation= with uniform_ratio=True (the single-gather form w = u_n + kappa v_n) is not supported")
        c_cells, rho_cells = per_cell(speed_of_sound, mesh, "speed_of_sound"), per_cell(density, mesh, "density")
        beta_cells = per_cell(nonlinear_coefficient, mesh, "nonlinear_coefficient")
        att_cells = per_cell(attenuation_coefficient_dB, mesh, "attenuation_coefficient_dB")
        bd1, bd2, D, G_d, detJ_d, (dF1_d, dF2_d) = self._init_common(mesh, float_type, comm, fused, source_time)
        self._init_relaxation(relaxation)
        self.f0 = float(source_frequency)
        self.w0 = 2 * np.pi * self.f0
        self._init_terms(sponge, point_source, point_claim)
        pick = (lambda a: float(a[bd1[:, 0]].mean())) if bd1.shape[0] else (lambda a: float(a.mean()))
        self.c0 = float(reference_speed_of_sound) if reference_speed_of_sound is not None else (
            float(speed_of_sound) if np.ndim(speed_of_sound) == 0 else pick(c_cells))
        self.rho0 = float(reference_density) if reference_density is not None else (
            float(density) if np.ndim(density) == 0 else pick(rho_cells))
        self.p0 = float(source_amplitude) if source_amplitude is not None else self.rho0 * self.c0 * 0.38557513826589934
        self.beta = float(beta_cells.mean())
        delta_cells = compute_diffusivity_of_sound(self.w0, c_cells, att_cells)
        if nodal_medium is not None:  # the means of the nodal fields (delta is not linear in c: the mean of delta, not delta of the means)
            delta_cells = cell_means(self.delta_nodal, mesh.dofmap)
            fd1 = mesh.facet_dofmap(bd1)
            if bd1.shape[0] and reference_speed_of_sound is None:
                self.c0 = float(self.c_nodal[fd1].mean())
            if bd1.shape[0] and reference_density is None:
                self.rho0 = float(self.rho_nodal[fd1].mean())
            self.p0 = float(source_amplitude) if source_amplitude is not None else self.rho0 * self.c0 * 0.38557513826589934
        self.delta = float(delta_cells.mean())
        # per cell, in the mesh's cell order: what field_monitor.heat_deposition forms kappa = delta / (rho c^4) from
        self.delta_cells, self.rho_cells, self.c_cells = delta_cells, rho_cells, c_cells
        P, n, dev, ft = self.P, self.P + 1, self.dev, self.tdt_np
        rho, c, beta, delta = rho_cells, c_cells, beta_cells, delta_cells
        td = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=ft))).to(dev)  # noqa: E731
        # cuda/demo_nonlinear_bowl.py:357-374
        self.cc1 = td(1.0 / rho / c / c)
        self.cc2 = td(-2.0 * beta / rho / rho / c**4)
        self.cc3 = td(-1.0 / rho)
        self.cc4 = td(-delta / rho / c / c)
        self.cc5 = td(2.0 * beta / rho / rho / c**4)
        c1, c2 = bd1[:, 0], bd2[:, 0]
        self.fc1_1 = td(1.0 / rho[c1])
        self.fc2_1 = td(delta[c1] / rho[c1] / c[c1] ** 2)
        self.fc1_2 = td(delta[c2] / rho[c2] / c[c2] ** 3)
        self.fc2_2 = td(-1.0 / rho[c2] / c[c2])
        if nodal_medium is not None:
            # the medium sits in nodal factors: unit cell constants (-1 for both stiffness inputs), one mean per facet; cc2 / cc5 are
            # not applied (w2 / w5 come from M(1) 1)
            rn, cn, bn, dn = self.rho_nodal, self.c_nodal, self.beta_nodal, self.delta_nodal
            fd2 = mesh.facet_dofmap(bd2)
            self.cc1 = td(np.ones(mesh.ncells))
            self.cc3 = td(np.full(mesh.ncells, -1.0))
            self.cc4 = td(np.full(mesh.ncells, -1.0))
            self.cc2 = self.cc5 = None
            self.fc1_1 = td(facet_means(1.0 / rn, fd1))
            self.fc2_1 = td(facet_means(dn / rn / cn**2, fd1))
            self.fc1_2 = td(facet_means(dn / rn / cn**3, fd2))
            self.fc2_2 = td(-facet_means(1.0 / rn / cn, fd2))
            self._kappa3, self._kappa4 = td(1.0 / rn), td(dn / rn / cn**2)
            self._f0, self._f2 = td(1.0 / rn / cn**2), td(-2.0 * bn / rn**2 / cn**4)
        self.G, self.detJ = G_d, detJ_d
        self.dofmap = torch.from_numpy(mesh.dofmap).to(dev)
        self.dF1, self.dF2 = dF1_d, dF2_d
        self.fdm1 = torch.from_numpy(mesh.facet_dofmap(bd1)).to(dev)
        self.fdm2 = torch.from_numpy(mesh.facet_dofmap(bd2)).to(dev)
        # the fused stage's facet sets: M_f1(fc1_1 g + fc2_1 dg) 1 with (g, dg) = source_values(t) -- or, with a phased-array source
        # (sources.py), g = 2 p0 w0 / c0 per element and its derivative through fus_facet_source_array_* -- and M_f2(fc2_2) v_n
        self._init_source(source, bd1, 2.0 * self.p0 * self.w0 / self.c0, (self.fc1_1, self.fc2_1, self.dF1, self.fdm1))
        self._absorbing_set = (self.fc2_2, self.dF2, self.fdm2)
        self.stiff = ops.stiffness_operator(P, D.flatten(), ft)
        # detJ never changes in the life of a solver: the reference-sequence stage applies the cell mass operator twice per stage
        # with it (cuda/demo_nonlinear_bowl.py:612-616, 630-632) -- streamed from a row-ordered copy instead of gathered
        self.mass_cell = ops.mass_operator(n**3, ft, static_detJ=not self.fused)
        self.mass_facet = ops.mass_operator(n * n, ft)
        self.axpy = ops.axpy(self.ndofs)
        # the reverse closures of the set-up exchange of the three assembled diagonals (m0, w2, w5) with the others
        # (the reference launch sequence with relaxation mechanisms scatters ur beside u_n, which the lumped mass still reads)
        self.fwd_v, self.fwd_w, *more = self._init_halo(halo_plan, forward=2 if relaxation is None else 3, reverse=2, overlap=overlap)
        self.fwd_r = more[0] if more else None
        if self.halo is not None:
            self.fwd_u, self.rev_m = self.halo.fwd, self._rev_setup[1]
        z = lambda: torch.zeros(self.ndofs, dtype=self.tdt, device=dev)  # noqa: E731
        (self.u, self.v, self.u0, self.v0, self.un, self.vn, self.ku, self.kv, self.u_n, self.v_n, self.w_n,
         self.g, self.dg, self.b, self.m, self.m0) = (z() for _ in range(16))
        # steady part of the lumped mass (:458-475)
        ops.fill(1.0, self.g)
        # set-up applies on the default operator (atomic-free, bitwise reproducible), like the reference-sequence stage's two
        # cell mass applies: each runs alone on this stream, the reverse scatters follow in stream order
        self.mass_cell(self.g, self.cc1, self.m0, self.detJ, self.dofmap)
        if nodal_medium is not None:
            # m0 holds this rank's part of M(1) 1: the three diagonals are that times a nodal factor.  Ghost values of the factors agree
            # across ranks (NodalMedium's contract), so the factor is applied BEFORE the reverse scatter and the one grouped exchange stays
            self.w2, self.w5 = self.m0 * self._f2, z()
            self.w5.sub_(self.w2)
            self.m0.mul_(self._f0)
        self.mass_facet(self.g, self.fc1_2, self.m0, self.dF2, self.fdm2)

        self.cell_fused = ops.westervelt_cell_operator(P, D.flatten(), ft)
        # fused mode: with GLL collocation the mass operator is diagonal, M(c) x = diag(M(c) 1) x, so the
        # stage's two cell mass applies (M(c2) u_n for the lumped mass, M(c5) v_n^2 for the right-hand side,
        # cuda/demo_nonlinear_bowl.py:612-616,630-632) are pointwise products with two diagonals assembled
        # once, like m0; the cell pass is then the stiffness part alone and m needs no reverse scatter
        if nodal_medium is None:
            self.w2, self.w5 = z(), z()
            self.mass_cell(self.g, self.cc2, self.w2, self.detJ, self.dofmap)  # g == 1 here
            self.mass_cell(self.g, self.cc5, self.w5, self.detJ, self.dofmap)
        # the reverse scatters of the three assembled diagonals, as one grouped exchange
        self._start_setup(defer_setup_exchange)
        # uniform ratio c4 / c3 (= delta / c^2: every homogeneous medium): K(c3) u + K(c4) v = K(c3)(u + kappa v),
        # so the cell pass CAN be one plain stiffness apply on w = u_n + kappa v_n, which the vector kernel writes (uniform_ratio=True)
        ratio = self.cc4 / self.cc3
        kmin, kmax = float(ratio.min().item()), float(ratio.max().item())
        # the decision (and kappa itself) must be the SAME on every rank -- a rank in single-gather mode forward-scatters
        # w where a neighbour in two-gather mode expects u_n, with matching counts, so nothing would hang and the result
        # would be silently wrong: min / max over all ranks (the ranks of one process decide locally).  cc3 / cc4 must not be
        # edited after construction.
        if not getattr(self.comm, "in_process", False):
            from .scatterer import gather_floats

            every = gather_floats(self.comm, [kmin, kmax])
            kmin, kmax = float(every[:, 0].min()), float(every[:, 1].max())
        self.kappa = kmin if abs(kmax - kmin) <= 1e-14 * max(abs(kmin), abs(kmax), 1e-300) else None
        # Which form: since the vector pass streams with non-temporal accesses (round 4) the TWO-gather cell pass is the faster one --
        # the single-gather form pays for writing w in the vector pass and re-reading it: P = 6, 36^3 cells, paired: 1.285 against
        # 1.458 ms per step with in-kernel geometry, 1.538 against 1.593 with the G array (profiles/r05i_ab_westervelt_gathers.log).
        # "auto" / False: two gathers; True: the single-gather form where the medium allows it.
        if uniform_ratio is not True:
            self.kappa = None
        self.w = z() if self.kappa is not None else None
        # opt-in (fused mode): G and detJ formed in the cell kernel from the vertices -- the cells of
        # the reference's meshes are trilinear (P1 geometry, cuda/demo_nonlinear_bowl.py:317)
        if nodal_medium is not None:
            in_kernel_geometry = True  # at every degree, and in the reference launch sequence too: the nodal kernels form G themselves
        elif in_kernel_geometry == "auto":
            in_kernel_geometry = self.fused and P >= IN_KERNEL_GEOMETRY_FROM_DEGREE
        self.in_kernel_geometry = bool(in_kernel_geometry)
        if self.in_kernel_geometry and self.fused and not keep_G:
            self.G = None  # the fused stage does not read it (P = 6, 36^3 cells: 768 MB)
        stiff, pair = self.stiff, self.cell_fused
        if self.in_kernel_geometry:
            geometry = vertex_geometry(mesh, P, dev)
            self.x_dofs = geometry[0]
            self.cell_fused_geom = ops.westervelt_cell_operator(P, D.flatten(), ft, geometry=geometry[1:])
            self.stiff_geom = ops.stiffness_operator(P, D.flatten(), ft, geometry=geometry)
            stiff, pair = self.stiff_geom, self.cell_fused_geom
        self.nodal_cell_pass = None
        if nodal_medium is not None:
            self.nodal_cell_pass = NODAL_CELL_PASS_DEFAULT if nodal_cell_pass == "auto" else nodal_cell_pass
            self.cell_nodal = ops.westervelt_cell_operator(P, D.flatten(), ft, geometry=geometry[1:], nodal=(self._kappa3, self._kappa4))
            self.stiff_nodal3 = ops.stiffness_operator(P, D.flatten(), ft, geometry=geometry, nodal=self._kappa3)
            self.stiff_nodal4 = ops.stiffness_operator(P, D.flatten(), ft, geometry=geometry, nodal=self._kappa4)
            pair = self.cell_nodal
        # the fused stage's cell pass, one of four: single gather (K(c3) w, w = u_n + kappa v_n) or two (K(c3) u_n + K(c4) v_n),
        # each with the G array or G formed in the kernel (x_dofs rows travel in the G position)
        self._percell = (self.cc3, self.cc4, self.x_dofs if self.in_kernel_geometry else self.G, self.dofmap)
        if self.nodal_cell_pass == "two-launch":
            def two_launches(u_n, v_n, c3, c4, G_, dm_):
                self.stiff_nodal3(u_n, c3, self.b, G_, dm_)
                self.stiff_nodal4(v_n, c4, self.b, G_, dm_)

            self._cell_pass = two_launches
        elif self.kappa is not None:
            self._cell_pass = lambda u_n, v_n, c3, c4, G_, dm_: stiff(self.w, c3, self.b, G_, dm_)
        else:
            self._cell_pass = lambda u_n, v_n, c3, c4, G_, dm_: pair.stiffness_only(u_n, v_n, c3, c4, self.b, G_, dm_)
        # the attachment writes self.cc4 -- the array object _percell and the reference launch sequence hold -- from this copy
        self.shock_capture = shock_capture
        if shock_capture is not None:
            self.cc4_base = shock_capture.bind(self)._base

    def init(self):
        super().init()
        if self.shock_capture is not None:
            self.shock_capture.reset()

    def setup_schedule(self):
        yield from self._reverse_setup((self.m0, self.w2, self.w5))
        self._bind_terms(self.m0)  # m0 is complete only now
        yield from self._bind_relaxation()

    def source_values(self, t):
        """g and dg/dt (cuda/demo_nonlinear_bowl.py:560-595)."""
        T, alpha = 1.0 / self.f0, 4.0
        if t < T * alpha:
            window = 0.5 * (1.0 - np.cos(self.f0 * np.pi * t / alpha))
            dwindow = 0.5 * np.pi * self.f0 / alpha * np.sin(self.f0 * np.pi * t / alpha)
        else:
            window, dwindow = 1.0, 0.0
        a = 2.0 * self.p0 * self.w0 / self.c0
        g = window * a * np.cos(self.w0 * t)
        dg = dwindow * a * np.cos(self.w0 * t) - window * a * self.w0 * np.sin(self.w0 * t)
        return g, dg

    def _source_scalars(self, t):
        return self.source_values(t)

    # -- fused stage: one cell pass + one vector pass ------------------------------------------------
    def _cell_terms(self, u_n, v_n, facets):
        """The cell pass chosen at construction into b, then ``facets()``; next to a halo the interior cells overlap the
        exchange of (w or u_n, v_n) and the reverse scatter of b follows."""
        cells = lambda *percell: self._cell_pass(u_n, v_n, *percell)  # noqa: E731
        if self.halo is None:
            cells(*self._percell)
            facets()
        else:
            yield from self.halo.schedule(cells, self._percell, [(self.fwd_u, self.w if self.kappa is not None else u_n), (self.fwd_v, v_n)],
                                          [(self.halo.rev, self.b)], facets)

    def _stiffness_operator(self):
        """K(-1/rho) of u alone, with the operator this solver holds for it (``solver_base._stiffness_of``: the energy record and
        ``stable_time_step``): the nodal kernel, G formed in the kernel where the fused stage does so, else the G array."""
        if self.nodal_medium is not None:
            return self.stiff_nodal3, self.cc3, self.x_dofs, self.dofmap
        if self.in_kernel_geometry and self.fused:
            return self.stiff_geom, self.cc3, self.x_dofs, self.dofmap
        return self.stiff, self.cc3, self.G, self.dofmap

    def _energy_mass(self):
        """The steady lumped mass m0: the energy of the linear part."""
        return self.m0

    def _diffusive_ratio(self):
        if self.nodal_medium is not None:
            return float(np.max(self.delta_nodal / self.c_nodal**2))
        if self.shock_capture is not None:  # the worst case: every cell at its largest artificial diffusivity
            return float(np.max((self.delta_cells + self.shock_capture.eps_max) / self.c_cells**2))
        return float(np.max(self.delta_cells / self.c_cells**2))

    def _vector_pass(self, bw, aw, new_step):
        fn = getattr(_lib.load(), f"fus_rk4_stage_nl2_{_lib.suffix(self.tdt)}")
        _lib.check(
            fn(float(bw), float(aw), int(new_step), self.m0.data_ptr(), self.w2.data_ptr(), self.w5.data_ptr(),
               self.b.data_ptr(), self.u.data_ptr(), self.v.data_ptr(), self.u0.data_ptr(), self.v0.data_ptr(),
               self.ku.data_ptr(), self.un.data_ptr(), float(self.kappa or 0.0),
               self.w.data_ptr() if self.w is not None else None, self.nlocal, self.ndofs, _lib.stream_ptr()),
            "fus_rk4_stage_nl2",
        )

    def _fused_enter(self):
        ops.fill(1.0, self.g)  # source enters through scaled facet constants
        super()._fused_enter()
        if self.kappa is not None:
            ops.copy(self.u0, self.w)
            self.axpy(self.kappa, self.v0, self.w)

    def _graph_state(self):
        return super()._graph_state() + ((self.w,) if self.w is not None else ())

    # -- reference launch sequence (blocking scatters: never yields) ---------------------------------
    def _stage_reference(self, i, t, dt):
        copy, fill, axpy = ops.copy, ops.fill, self.axpy
        copy(self.u0, self.un)
        copy(self.v0, self.vn)
        axpy(A_RUNGE[i] * dt, self.ku, self.un)
        axpy(A_RUNGE[i] * dt, self.kv, self.vn)
        copy(self.vn, self.ku)
        ts = self._stage_time(t, i, dt)
        if self.source is None:  # the reference's own launches: g and dg filled into vectors, then their facet mass applies
            gv, dgv = self.source_values(ts)
            fill(gv, self.g)
            fill(dgv, self.dg)

            def source_facets():
                self.mass_facet(self.g, self.fc1_1, self.b, self.dF1, self.fdm1)
                self.mass_facet(self.dg, self.fc2_1, self.b, self.dF1, self.fdm1)
        else:  # the array's g and dg terms in one launch (no set B) replace all four
            source_facets = lambda: self._facet_source.launch(self.b, None, t=ts)  # noqa: E731
        copy(self.un, self.u_n)
        copy(self.vn, self.v_n)
        ops.square(self.vn, self.w_n)
        if self.halo is not None:
            self.fwd_u(self.u_n)
            self.fwd_v(self.v_n)
            self.fwd_w(self.w_n)
            if self.relaxation is not None:
                self.fwd_r(self._relax_bound().ur)
        nl = self.nlocal
        if self.nodal_medium is not None:
            # nodal medium: the two cell mass applies are pointwise products with the assembled diagonals (complete at the owned dofs:
            # no reverse scatter of m), the stiffness part two launches of the nodal stiffness operator
            copy(self.m0, self.m)
            ops.muladd(self.w2, self.u_n, self.m[:nl])
            fill(0.0, self.b)
            self.stiff_nodal3(self._stiffness_input(self.u_n), self.cc3, self.b, self.x_dofs, self.dofmap)
            self.stiff_nodal4(self.v_n, self.cc4, self.b, self.x_dofs, self.dofmap)
            ops.muladd(self.w5, self.w_n, self.b[:nl])
        else:
            # unsteady lumped mass
            fill(0.0, self.m)
            self.mass_cell(self.u_n, self.cc2, self.m, self.detJ, self.dofmap)
            if self.halo is not None:
                self.halo.rev(self.m)
            axpy(1.0, self.m0, self.m)
            # right-hand side
            fill(0.0, self.b)
            self.stiff(self._stiffness_input(self.u_n), self.cc3, self.b, self.G, self.dofmap)
            self.stiff(self.v_n, self.cc4, self.b, self.G, self.dofmap)
            self.mass_cell(self.w_n, self.cc5, self.b, self.detJ, self.dofmap)
        source_facets()
        self.mass_facet(self.v_n, self.fc2_2, self.b, self.dF2, self.fdm2)
        self._extra_terms(self.u_n, self.v_n, ts)
        if self.halo is not None:
            self.halo.rev(self.b)
        if self.nodal_medium is not None:  # m is formed at the owned dofs only
            ops.pointwise_divide(self.b, self.m, self.kv[:nl])
        else:
            ops.pointwise_divide(self.b, self.m, self.kv)
        axpy(B_RUNGE[i] * dt, self.ku, self.u)
        axpy(B_RUNGE[i] * dt, self.kv, self.v)
        self._relax_reference(i, dt)
        yield from ()  # the base class's stage protocol is a generator; this sequence has nothing to post
