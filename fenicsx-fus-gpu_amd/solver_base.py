"""
The explicit RK4 time loop both wave solvers share (``LinearSpectral3D``, ``WesterveltSpectral3D``): their common set-up,
the step loop of ``rk4`` / ``rk4_schedule``, the fused step and its hipGraph replay (``rk4_graph``).  A solver supplies its
physics through hooks:

  ``setup_schedule()``                  generator: the set-up exchange (reverse scatters of the assembled mass)
  ``_stage_reference(i, t, dt)``        generator: stage ``i`` as the reference's launch sequence
  ``_cell_terms(u_n, v_n, facets)``     generator: the cell part of a fused stage into ``b``, then ``facets()``
  ``_vector_pass(bw, aw, kind)``        the fused stage's vector kernel (csrc/rk4.hpp)
  ``_source_scalars(t)``                ``(s1, s2)`` of the scalar source facet term at time ``t``
  ``_absorbing_set``                    ``(c, detJ, dofmap)`` of the absorbing facet set (set B of the facet launch)

and, in its constructor, ``_init_source(source, facets, scale, source_set)`` and ``_init_terms(sponge, point_source, point_claim)``;
at the end of ``setup_schedule``, when its lumped mass is complete, ``_bind_terms(mass)``.

The source-facet term is one SOURCE OBJECT, ``self._facet_source``: ``sources.ScalarFacetSource`` (set A, ``(c1, c2 or None, detJ,
dofmap)``, with ``_source_scalars``) or the ``sources.BoundSourceArray`` of ``source=``.  It answers ``stage_row(t)`` (the host row of
a stage time), ``stage_slot(dtype, device)`` (the zeroed [4, width] device tensor a captured step reads) and ``launch(b, field, t=None,
slot=None)`` (set A with set B in one launch).  What is ADDED to a stage's right-hand side besides is a list of STAGE TERMS,
``self._terms``: objects with ``bind(solver, mass)``, ``launch(b, u_n, v_n, t)`` and ``capturable`` (``refusal`` says why not).  The
sponge layer (``sponge=``, sponge.SpongeTerm: one sparse launch over the layer's owned dofs) and the point sources (``point_source=``,
sources.BoundPointSources: one launch at the stage's source time) are the two, in this order; ``_extra_terms(u_n, v_n, t)`` launches
them after the facet launch, in ``facets()`` of the fused stage and after the facet applies in ``_stage_reference``.  Relaxation is not
a stage term: it replaces the stiffness input and adds a pass on either side of the vector pass, so it keeps hooks of its own.

With ``relaxation=`` (power-law absorption through relaxation mechanisms, relaxation.py) every stiffness apply of a stage acts on
``self._relax.ur = u_n + sum xi`` in the place of ``u_n`` (``_stiffness_input``; on a partitioned mesh ``ur`` is what travels), and a
stage has one more streaming launch, ``_relax_pass``: before the vector pass in stages 1-3 (it reads ``u0`` and the stage's ``v_n``,
which that pass overwrites), after it in stage 4 (it reads the new ``u0``).  A solver calls ``_init_relaxation`` in its constructor and
``yield from self._bind_relaxation()`` at the end of ``setup_schedule`` (the per-dof weights are a lumped projection: its reverse
exchange).  The lumped mass, the quadratic term, the facet terms, the sponge and the point sources still see ``u_n`` and ``v_n``.

``rk4_schedule`` and ``rk4_graph`` record through one hook, ``_recording`` (the steps and their factors: ``recording.py``);
``run_schedule`` drives one rank's schedule generator to its value (``rk4``, ``bioheat.py``, ``field_monitor.py``), ``run_lockstep``
those of several ranks of one process.  ``MeshSolver3D`` is the set-up these solvers share with ``bioheat.py``.

hipGraph replay of the fused step (single rank) is for meshes small enough that the launches, not the kernels, bound the
step -- below roughly 0.5 M dofs when driven from Python (tools/time_rk4_graph.py: 1.7x at 50 k dofs, 1.4x at 118 k,
nothing to gain from 1 M dofs up, where consecutive stream launches overlap their tails and graph nodes do not).  Every
launch of a fused step takes fixed device pointers and constants except the source values g(t), dg/dt of the boundary-facet
terms; with ``fus_facet_terms_dev_*`` those are read from device memory, so the step is captured once
(``torch.cuda.CUDAGraph`` = hipStreamBeginCapture / hipGraphLaunch) and replayed with one 16-byte-per-stage device copy of
the step's source values into ``_stage_slot``.  A solver with a phased-array source (``self.source``, sources.py) reads a fp64
stage block per stage instead (``fus_facet_source_array_dev_*``): its slot is [4, 6], rewritten before each replay in the
same way.  The reference drives every launch from Python (cuda/demo_linear_box.py:487-566: 12 launches + 5 host syncs per
stage); this is its launch-bound regime taken to one graph launch per step.
"""

from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from . import operators as ops
from .gll import gll_points_weights, tabulate_1d, tensor_points_3d, tensor_weights_2d, tensor_weights_3d
from .precompute import (
    compute_boundary_facets_scaled_jacobian_determinant_device,
    compute_scaled_geometrical_factor_device,
    tabulate_facet_gradients,
    tabulate_hex_p1_gradients,
)
from .recording import rk4_steps  # also for bioheat.py and the tests, which take it from here
from .sources import ScalarFacetSource
from .sponge import SpongeTerm

A_RUNGE = (0.0, 0.5, 0.5, 1.0)
B_RUNGE = (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)
C_RUNGE = (0.0, 0.5, 0.5, 1.0)


def per_cell(value, mesh, name):
    """A material parameter as a per-cell array in the MESH's cell order: a scalar (homogeneous medium, the reference's box
    demos) or one value per cell in the caller's cell order (the DG0 arrays ``c0.x.array`` ... of the reference's production
    drivers, cuda/demo_nonlinear_bowl.py:166-178; a mesh that re-ordered its cells -- ``ArrayMesh`` -- permutes them)."""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        return np.full(mesh.ncells, float(a))
    if a.shape != (mesh.ncells,):
        raise ValueError(f"{name}: a scalar or one value per cell ({mesh.ncells}), got shape {a.shape}")
    return np.ascontiguousarray(mesh.permute_cells(a) if hasattr(mesh, "permute_cells") else a)


def _to(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_facet_detJ(mesh, P, ft, dev, facet_sets, gm=None):
    """The scaled facet detJ of each of the given boundary_data sets (``(cell, local facet)`` rows), computed on the device;
    ``gm``: ``(x_dofs, x_g)`` on the device where the caller holds them (the solvers' set-up; ``receivers.ElementReceivers``
    does not)."""
    n, td = P + 1, _to(dev)
    pts, wts, _ = tabulate_1d(P, ft)
    gm = (td(mesh.x_dofs), td(mesh.x_g)) if gm is None else gm
    dphi_f, w2 = td(tabulate_facet_gradients(pts, ft)), td(tensor_weights_2d(wts).astype(ft))
    out = []
    for bd in facet_sets:
        dF = torch.zeros((bd.shape[0], n * n), dtype=_lib.torch_dtype(ft), device=dev)
        if bd.shape[0]:
            compute_boundary_facets_scaled_jacobian_determinant_device(dF, gm, td(bd.astype(np.int32)), dphi_f, w2)
        out.append(dF)
    return out


def device_geometry(mesh, P, ft, dev, facet_sets):
    """G, detJ and the facet detJ of the given boundary_data sets, computed on the device
    (csrc/geometry.hpp; the reference does this with numba on the host,
    cuda/demo_linear_box.py:245-317)."""
    n, td, tdt = P + 1, _to(dev), _lib.torch_dtype(ft)
    pts, wts, D = tabulate_1d(P, ft)
    gm = (td(mesh.x_dofs), td(mesh.x_g))
    G = torch.empty((mesh.ncells, n**3, 6), dtype=tdt, device=dev)
    detJ = torch.empty((mesh.ncells, n**3), dtype=tdt, device=dev)
    compute_scaled_geometrical_factor_device(G, gm, mesh.ncells, td(tabulate_hex_p1_gradients(tensor_points_3d(pts), ft)),
                                             td(tensor_weights_3d(wts).astype(ft)), detJ=detJ)
    return D, G, detJ, device_facet_detJ(mesh, P, ft, dev, facet_sets, gm)


# in_kernel_geometry="auto": from this degree; below it G is not the dominant stream and the kernel form loses
IN_KERNEL_GEOMETRY_FROM_DEGREE = 3


def vertex_geometry(mesh, P, dev):
    """``(x_dofs on the device, x_g, pts, wts)``: what an operator that forms G in the kernel from the 8 vertices of each cell is
    built with (the reference's geometry is P1 everywhere, cuda/demo_nonlinear_bowl.py:317)."""
    return (torch.from_numpy(np.ascontiguousarray(mesh.x_dofs)).to(dev), mesh.x_g) + gll_points_weights(P)


def stiffness_form(mesh, P, D, G, float_type, affine="auto", in_kernel_geometry="auto", keep_G=False, nodal=None):
    """The stiffness operator of ``LinearSpectral3D`` / ``BioheatSpectral3D``: ``(operator, what travels in the G position of its
    call, affine, in_kernel_geometry, G_array)``.  Affine cells (every box mesh of the reference's demos): the constant-G fast path,
    after checking that the geometry factors really are affine (``"auto"``), or on request / never.  Otherwise, on request or by
    ``IN_KERNEL_GEOMETRY_FROM_DEGREE``: G formed in the kernel; the rows of ``x_dofs`` then travel in the G position (cell sub-ranges
    slice them) and ``G_array``, the reference's array, is ``None`` unless ``keep_G`` (6 n^3 values per cell: 945 MB at config 3).
    ``nodal``: a coefficient per local dof inside the contraction (nodal_medium.py) -- the nodal kernel with G formed in the kernel, at
    every degree and on affine boxes too (an affine box is a trilinear mesh), unless ``in_kernel_geometry`` is ``False``: then the
    general kernel on the G array scaled once (``nodal_medium.scale_G``), which is what travels and what ``G_array`` is.  The
    constant-G path reads one record per cell and cannot carry it: ``affine=True`` raises."""
    ft = np.dtype(float_type)
    if nodal is not None:
        if affine is True:
            raise ValueError("affine=True with a nodal medium: the affine fast path reads one geometric record per cell, a nodal "
                             "coefficient varies inside the cell")
        if in_kernel_geometry is False:
            from .nodal_medium import scale_G

            Gs = scale_G(G, nodal, mesh.dofmap)
            return ops.stiffness_operator(P, D.flatten(), ft), Gs, False, False, Gs
        geometry = vertex_geometry(mesh, P, G.device)
        return ops.stiffness_operator(P, D.flatten(), ft, geometry=geometry, nodal=nodal), geometry[0], False, True, G if keep_G else None
    w3 = tensor_weights_3d(gll_points_weights(P)[1])
    affine = bool(affine) if affine != "auto" else ops.is_affine_geometry(G, w3, rtol=1e-11 if ft == np.float64 else 1e-5)
    if in_kernel_geometry == "auto":
        in_kernel_geometry = P >= IN_KERNEL_GEOMETRY_FROM_DEGREE
    if affine or not in_kernel_geometry:
        return ops.stiffness_operator(P, D.flatten(), ft, affine_weights=w3 if affine else None), G, affine, False, G
    geometry = vertex_geometry(mesh, P, G.device)
    return ops.stiffness_operator(P, D.flatten(), ft, geometry=geometry), geometry[0], False, True, G if keep_G else None


def run_schedule(gen):
    """Run one rank's schedule generator (it yields whenever the rank has posted halo exchanges) to exhaustion; returns its value."""
    while True:
        try:
            next(gen)
        except StopIteration as done:
            return done.value


def run_lockstep(gens):
    """Advance the generators of several in-process ranks together: each ``next`` runs a rank up to the point
    where it has posted a set of halo exchanges; results are the generators' return values."""
    out = [None] * len(gens)
    live = list(enumerate(gens))
    while live:
        nxt = []
        for i, g in live:
            try:
                next(g)
                nxt.append((i, g))
            except StopIteration as done:
                out[i] = done.value
        live = nxt
    return out


class MeshSolver3D:
    """What a solver does before its first step: communicator, device, dtype, geometry, halo closures and the set-up exchange."""

    def _init_mesh(self, mesh, float_type, comm, facet_sets=()):
        """The attributes every solver sets first; returns ``device_geometry``: ``D, G, detJ, [facet detJ of each set]``."""
        if comm is not None:  # an MPI.Comm (the reference's comm = MPI.COMM_WORLD) becomes the bootstrap of a NativeComm
            from .scatterer import as_comm

            comm = as_comm(comm)
        self.comm, self.mesh, self.P = comm, mesh, mesh.P
        self.nlocal, self.ndofs = mesh.nlocal, mesh.ndofs
        self.tdt_np, self.tdt = np.dtype(float_type), _lib.torch_dtype(float_type)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        return device_geometry(mesh, self.P, self.tdt_np, self.dev, facet_sets)

    def _init_halo(self, halo_plan, forward=0, reverse=0, overlap=True, kernels=None):
        """``self.halo`` around ``self.stiff`` (``None`` on one rank), ``forward`` more forward closures (returned) and ``reverse``
        more reverse ones (``self._rev_setup``: ``halo.rev`` and those, one per vector of the set-up exchange).  ``halo_plan =
        (owners_data, ghosts_data)`` computed elsewhere (a host that drives several ranks from one process has no index exchange
        to run); default: exchanged over ``comm`` now.  Every closure is built HERE, at construction: building one is a collective
        step of the PEER transport (arena handles), and ranks driven from one process must all have built theirs before any exchanges."""
        self.halo, self._rev_setup = None, []
        if self.comm is None or self.comm.size == 1:
            return [None] * forward
        from .scatterer import HaloApply, scatter_forward, scatter_reverse

        self.halo = HaloApply(self.mesh, self.stiff, self.comm, self.tdt_np, overlap=overlap, kernels=kernels, plan=halo_plan)
        make = lambda scatter, k=None: scatter(self.comm, self.halo.owners_data, self.halo.ghosts_data, self.nlocal, self.tdt_np, k)  # noqa: E731
        more = [make(scatter_forward, kernels) for _ in range(forward)]
        self._rev_setup = [self.halo.rev] + [make(scatter_reverse) for _ in range(reverse)]
        return more

    def _start_setup(self, defer_setup_exchange):
        """The set-up exchange (``setup_schedule``): now, or -- several ranks driven from one process, every rank must have
        posted before any completes -- by the driver through ``self._setup``."""
        self._setup = self.setup_schedule()
        if not defer_setup_exchange:
            run_schedule(self._setup)

    def _reverse_setup(self, vectors):
        """Generator: post the reverse scatters of the assembled ``vectors`` (one per closure of ``self._rev_setup``), yield, complete."""
        if self.halo is not None:
            from .scatterer import begin_all

            pending = begin_all(zip(self._rev_setup, vectors, strict=True))
            yield "reverse"
            for sc, vec, wk in pending:
                sc.end(vec, wk)

    def check_halo_health(self, what="halo exchange"):
        if self.halo is not None:
            self.halo.check_health(what)


class SpectralSolver3D(MeshSolver3D):
    """The time loop of an explicit RK4 solver for u' = v, M v' = r(u, v, t) (see the module docstring for its hooks)."""

    def _init_common(self, mesh, float_type, comm, fused, source_time):
        """The attributes both wave solvers set first; returns the source and absorbing facet sets and the device geometry:
        ``bd1, bd2, D, G, detJ, (dF1, dF2)``."""
        self.fused, self.source_time = bool(fused), source_time
        # what stable_time_step() leaves: the two operator bounds and the unscaled RK4 limit they give (None until it has run)
        self.lambda_max = self.damping_max = self.stable_limit = None
        self._warned_step = False
        self.lean_stages = os.environ.get("FUS_RK4_LEAN", "1") != "0"  # the fused stage's vector pass: kinds 4-7 of csrc/rk4.hpp (_stage_args)
        # the two tagged facet sets (cuda/demo_linear_box.py:230-243, cuda/utils.py:81-114): a structured box names them by its
        # faces (x = 0: source, x = L: absorbing), a mesh handed over as arrays (dolfinx_adaptor.ArrayMesh) by its facet tags
        bd1 = mesh.boundary_facets([getattr(mesh, "source_tag", 2)])
        bd2 = mesh.boundary_facets([getattr(mesh, "absorbing_tag", 3)])
        return (bd1, bd2) + self._init_mesh(mesh, float_type, comm, (bd1, bd2))

    # -- the source-facet term: one source object, the scalar waveform or a phased array (sources.py) ----------------------------------
    def _init_source(self, source, facets, scale, source_set):
        """``source``: a ``sources.SourceArray`` or None, bound here to this rank's source ``facets`` with the source constant ``scale``
        (needs ``self.f0``) and set A, ``source_set = (c1, c2 or None, detJ, dofmap)``: ``self.source`` (None without an array).
        ``self._facet_source`` is what the stages launch either way: that, or the ``ScalarFacetSource`` of ``_source_scalars``."""
        c1, c2, detJ, dofmap = source_set
        self.source = None if source is None else source.bind(self.mesh, facets, self.tdt_np, self.dev, frequency=self.f0, scale=scale,
                                                              coeff1=c1, coeff2=c2, detJ=detJ, dofmap=dofmap)
        self._facet_source = ScalarFacetSource(source_set, self._source_scalars) if source is None else self.source

    # -- additive stage terms: the sponge layer (sponge.py), then the point sources (sources.PointSources) -----------------------------
    def _init_terms(self, sponge, point_source, point_claim=None):
        """``sponge``: a ``sponge.SpongeLayer`` or None.  ``point_source``: a ``sources.PointSources`` or None, bound here to the points
        this rank injects (needs ``self.f0``); ``point_claim``: this rank's row of ``sources.claim_points`` for ranks driven from one
        process (they have no gather)."""
        self.sponge, self.point_source = sponge, point_source
        self._sponge_term = None if sponge is None else SpongeTerm(sponge, self.mesh)
        self._points = None if point_source is None else point_source.bind(
            self.mesh, self.tdt_np, self.dev, self.f0, comm=self.comm, claim=point_claim)
        self._terms = [term for term in (self._sponge_term, self._points) if term is not None]

    @property
    def _sponge(self):
        """``(idx, cu, cv)`` of the bound layer; None without one, and until the set-up exchange has run."""
        return None if self._sponge_term is None else self._sponge_term.bound

    def _bind_terms(self, mass):
        """At the end of ``setup_schedule``: ``mass``, the solver's assembled lumped mass, is complete only then."""
        for term in self._terms:
            term.bind(self, mass)

    def _extra_terms(self, u_n, v_n, t):
        """The terms' launches of a stage with inputs ``(u_n, v_n)`` and source time ``t`` (None: a capture) into ``b``."""
        for term in self._terms:
            term.launch(self.b, u_n, v_n, t)

    # -- relaxation mechanisms (relaxation.RelaxationAbsorption): one streaming launch per stage, ur in the place of u_n ---------------
    def _init_relaxation(self, relaxation):
        """``relaxation``: a ``relaxation.RelaxationAbsorption`` or None.  Its state on the device needs the cell mass operator and, for
        per-cell weights on a partitioned mesh, a reverse exchange: it is bound in ``setup_schedule`` (``_bind_relaxation``)."""
        self.relaxation, self._relax = relaxation, None

    def _bind_relaxation(self):
        """Generator (it yields after posting each reverse exchange of the weights' lumped projection)."""
        if self.relaxation is not None:
            self._relax = yield from self.relaxation.bind_schedule(self)

    def _relax_bound(self):
        if self._relax is None:
            raise _lib.FusGpuError("relaxation: the set-up exchange (setup_schedule) has not run, the mechanisms are not bound yet")
        return self._relax

    def _stiffness_input(self, u_n):
        """What the stiffness applies of a stage act on: ``u_n``, or with relaxation mechanisms ``ur = u_n + sum xi``."""
        return u_n if self.relaxation is None else self._relax_bound().ur

    def _relax_pass(self, i, dt, u_base, vn):
        """The mechanisms' pass of stage ``i``: xi through the stage (FIRST, MIDDLE, MIDDLE, LAST) and the next stage's ``ur`` =
        ``u_base + a_{i+1} dt vn + sum xi`` (stage 4: ``u_base`` is the new u, nothing is added to it)."""
        aw = 0.0 if i == 3 else A_RUNGE[i + 1] * dt
        self._relax.stage(ops.RELAX_LAST if i == 3 else (ops.RELAX_FIRST if i == 0 else ops.RELAX_MIDDLE), B_RUNGE[i] * dt, aw, aw, u_base, vn)

    def _relax_reference(self, i, dt):
        """The pass in the reference launch sequence, at the end of stage ``i``: ``ku`` holds the stage's v_n, ``u`` the new u after stage 4."""
        if self.relaxation is not None:
            self._relax_pass(i, dt, self.u if i == 3 else self.u0, self.ku)

    def _check_relaxation_step(self, dt):
        if self.relaxation is not None:
            self.relaxation.check_time_step(dt)

    def init(self):
        """u = v = 0 (cuda/demo_linear_box.py:434-435); with relaxation mechanisms their memory variables too."""
        for t in (self.u, self.v, self.ku, self.kv):
            ops.fill(0.0, t)
        if self.relaxation is not None:
            self._relax_bound().zero()

    def _stage_time(self, t, i, dt):
        """The time stage ``i`` of the step from ``t`` evaluates its source at: the stage time (``source_time="tn"``) or,
        as the CUDA demos do, the step's start."""
        return t + C_RUNGE[i] * dt if self.source_time == "tn" else t

    def _stage_args(self, i, dt):
        """``(bw, aw, kind)`` of the vector pass after stage ``i`` (csrc/rk4.hpp).  Default: the LEAN set 4, 5, 6, 7 with bw = b_runge[0] dt,
        aw = a_runge[1] dt in all four passes (u's accumulator runs one pass ahead, 34 instead of 41 vector touches per linear step, 46
        instead of 52 per Westervelt step; v differs from the reference's sequence in the rounding of one term); ``lean_stages = False``
        (FUS_RK4_LEAN=0): kinds 2, 0, 0, 3, the reference's arithmetic operation for operation."""
        if self.lean_stages:
            return B_RUNGE[0] * dt, A_RUNGE[1] * dt, 4 + i
        last = i == 3
        return B_RUNGE[i] * dt, 0.0 if last else A_RUNGE[i + 1] * dt, 3 if last else (2 if i == 0 else 0)

    # -- fused stage: the cell pass with the facet terms in one launch, then one vector pass -------------------------------
    def _operator_fused(self, t, u_n, v_n, slot=None):
        """b += the cell terms of (u_n, v_n) + the facet terms of the source at time ``t`` and M_f2(c) v_n, in one facet
        launch, + the additive terms.  ``slot`` (graph capture, ``t`` is None): the device row the source's kernel reads its
        stage values from instead of their being evaluated at ``t``."""
        def facets():  # wherever a schedule (or a capture) places the facet launch, the terms' launches follow it
            self._facet_source.launch(self.b, (v_n,) + self._absorbing_set, t=t, slot=slot)
            self._extra_terms(u_n, v_n, t)

        yield from self._cell_terms(self._stiffness_input(u_n), v_n, facets)

    def _fused_step(self, t, dt):
        """The 8 launches of one fused RK4 step from ``t``: the first stage reads (u0, v0) themselves, the others the stage
        buffers (un, ku == v_n).  ``t=None`` (graph capture): every argument is a fixed pointer or a constant, the source
        values of stage ``i`` are read from ``self._stage_slot[i]``."""
        for i in range(4):
            u_n, v_n = (self.u0, self.v0) if i == 0 else (self.un, self.ku)
            if t is None:
                yield from self._operator_fused(None, u_n, v_n, slot=self._stage_slot[i])
            else:
                yield from self._operator_fused(self._stage_time(t, i, dt), u_n, v_n)
            if self.relaxation is not None and i < 3:  # before the vector pass overwrites the stage's v_n (and, lean stage 3, u0)
                self._relax_pass(i, dt, self.u0, v_n)
            self._vector_pass(*self._stage_args(i, dt))
            if self.relaxation is not None and i == 3:  # after it: u0 is the new u; neither LAST kind writes ku
                self._relax_pass(i, dt, self.u0, v_n)

    def _fused_enter(self):
        """Before a fused step loop: between steps the solution lives in (u0, v0), the first stage's inputs as they stand;
        the last stage writes the new solution straight into them."""
        ops.fill(0.0, self.b)
        ops.copy(self.u, self.u0)
        ops.copy(self.v, self.v0)
        if self.relaxation is not None:
            self._relax_bound().enter(self.u0)

    def _fused_exit(self):
        ops.copy(self.u0, self.u)
        ops.copy(self.v0, self.v)

    # -- the time loop -----------------------------------------------------------------------------------------------------
    def rk4(self, start_time, final_time, dt, max_steps=None, sensors=None, record_from=None, monitor=None, receivers=None, energy=None,
            guard=None):
        """Advance from ``start_time`` to ``final_time`` (cuda/demo_linear_box.py:487-566).
        Returns ``(t, steps)``.  ``sensors``: a ``sensors.PointSensors`` recorded after every step that ends after
        ``record_from`` (default: every step) while its series has room -- the supported way to observe the field mid-run.
        ``monitor``: a ``field_monitor.FieldMonitor`` that accumulates (u, v) over the owned dofs after the same steps (one
        launch, no exchange); it may be given together with ``sensors``.  ``receivers``: a ``receivers.ElementReceivers`` (the surface
        integral of the field over each element of an array, one launch) recorded after the same steps as the sensors.
        ``energy``: a ``diagnostics.EnergyRecorder`` (the conserved quadratic form after every ``every``-th of those steps: one
        stiffness apply and one reduction, no host sync).  ``guard``: a ``diagnostics.FieldGuard`` (every ``every`` steps ``max |u|``
        and the non-finite count are read back: ``FusGpuError`` when the field has blown up).  ``None`` leaves every launch as it is.
        A ``dt`` above the limit an earlier ``stable_time_step`` call found warns once; ``rk4`` never computes the limit itself."""
        result = run_schedule(self.rk4_schedule(start_time, final_time, dt, max_steps, sensors, record_from, monitor, receivers, energy,
                                                guard))
        # N > 1: every device-side wait of the exchange is bounded, so a late or dead neighbour cannot hang this
        # rank -- it must not hand back a field computed from stale ghosts either (the reference would block in
        # MPI Waitall, cuda/scatterer.py:175): raise.  One synchronisation per rk4() call.
        self.check_halo_health(f"{type(self).__name__}.rk4")
        return result

    def _warn_step(self, dt):
        if self.stable_limit is not None and dt > self.stable_limit and not self._warned_step:
            import warnings

            self._warned_step = True
            warnings.warn(f"{type(self).__name__}: dt = {dt:g} s exceeds the RK4 stability limit {self.stable_limit:g} s of this mesh and "
                          "medium (stable_time_step(safety=1)): the field will grow without bound", RuntimeWarning, stacklevel=4)

    def _recording(self, start_time, final_time, dt, max_steps, record_from, sensors, monitor, receivers, energy=None, guard=None):
        """Plan the recorders for this ``rk4`` call (``expect_steps``) and return ``record(t)``: the generator that records what is
        due after a step ending at ``t``.  On a partitioned mesh the ghost entries of the field are not current after a step: the
        forward exchange the sensors and the receivers read after is posted first -- once, if either is due -- with a ``yield`` after
        posting (the solvers' schedules post their stage exchanges the same way, so in-process lockstep drivers keep working); the
        monitor reads owned dofs only.  ``energy`` applies the stiffness to the field through the halo schedule (its own exchanges and
        yields); ``guard`` is asked after EVERY step, whatever ``record_from``.  A Westervelt solver's ``shock_capture`` attachment
        (shock_capture.py) launches its sensor last, after every step it is due, and shares the forward exchange."""
        self._warn_step(dt)
        for recorder in (sensors, monitor, receivers, energy, guard):
            if recorder is not None:
                recorder.expect_steps(start_time, final_time, dt, max_steps, record_from)
        rf = -np.inf if record_from is None else float(record_from)
        shock = getattr(self, "shock_capture", None)

        def record(t):
            u, v = (self.u0, self.v0) if self.fused else (self.u, self.v)
            if guard is not None:
                guard.check(self, u, t)
            sense = shock is not None and shock.due()  # after EVERY step, whatever record_from
            if not t > rf and not sense:
                return
            due = [r for r in (sensors, receivers) if r is not None and not r.full] if t > rf else []
            if due or sense:  # one exchange serves the recorders and the sensor launch
                if self.halo is not None:
                    wk = self.halo.fwd.begin(u)
                    yield "forward"
                    self.halo.fwd.end(u, wk)
                for r in due:
                    r.record(u, t)
            if t > rf:
                if monitor is not None:
                    monitor.record(u, v, t)
                if energy is not None:
                    yield from energy.record_schedule(u, v, t)
            if sense:  # after the recorders: they see the step as it was computed, cc4 changes for the steps that follow
                shock.launch(u)

        return record

    def rk4_schedule(self, start_time, final_time, dt, max_steps=None, sensors=None, record_from=None, monitor=None, receivers=None,
                     energy=None, guard=None):
        """``rk4`` as a generator that yields whenever this rank has posted halo exchanges (see
        ``HaloApply.schedule``); its return value is ``(t, steps)``.  A driver that advances several ranks' generators
        itself calls ``check_halo_health()`` when they are exhausted (``rk4`` does).  ``u`` / ``v`` are valid only once
        the generator is exhausted (the fused path keeps the solution in ``u0`` / ``v0`` between steps): observe the field
        mid-run through ``sensors`` (see ``rk4``; on a partitioned mesh a recording step posts a forward exchange of the
        field first, with a yield) or, over every owned dof, through ``monitor`` (no exchange, no yield)."""
        t, step = float(start_time), 0
        self._check_relaxation_step(dt)
        record = self._recording(t, final_time, dt, max_steps, record_from, sensors, monitor, receivers, energy, guard)
        if self.fused:
            self._fused_enter()
        elif self.relaxation is not None:
            self._relax_bound().enter(self.u)
        for t0, h in rk4_steps(t, final_time, dt, max_steps):
            if self.fused:
                yield from self._fused_step(t0, h)
            else:
                ops.copy(self.u, self.u0)
                ops.copy(self.v, self.v0)
                for i in range(4):
                    yield from self._stage_reference(i, t0, h)
            t, step = t0 + h, step + 1
            yield from record(t)
        if self.fused:
            self._fused_exit()
        return t, step

    # -- hipGraph replay (launch-bound meshes) -----------------------------------------------------------------------------
    def _graph_state(self):
        """The tensors a fused step mutates (saved / restored around the warm-up step of a capture)."""
        return (self.u, self.v, self.u0, self.v0, self.ku, self.un, self.b) + (self._relax_bound().state() if self.relaxation is not None else ())

    def _step_graph(self, dt):
        g = self._graphs.get(dt)
        if g is None:
            state = self._graph_state()
            saved = [t.clone() for t in state]
            # every kernel of the step once outside the capture (code objects load on first launch, batch
            # plans are built on first use), on state that is put back afterwards
            for _ in self._fused_step(None, dt):
                pass
            torch.cuda.synchronize()
            for t, s_ in zip(state, saved):
                t.copy_(s_)
            # the captured nodes hold the RAW device pointers of the batch-plan workspaces the operators looked up:
            # keep those workspaces (and the dofmaps they belong to) alive for as long as the graph lives -- the plan
            # cache is bounded and evicts oldest-first, and an evicted workspace that nothing else references would be
            # freed under the graph's feet (replay does not go through the plan registry)
            g = torch.cuda.CUDAGraph()
            ops._PLANS.start_recording()
            try:
                with torch.cuda.graph(g):
                    for _ in self._fused_step(None, dt):
                        pass
            finally:
                held = ops._PLANS.stop_recording()
            self._graphs[dt] = g
            self._graph_plans = getattr(self, "_graph_plans", {})
            self._graph_plans[dt] = held
        return g

    def rk4_graph(self, start_time, final_time, dt, max_steps=None, sensors=None, record_from=None, monitor=None, receivers=None,
                  energy=None, guard=None):
        """``rk4`` with the full-size steps replayed from ONE captured hipGraph.  Same kernels in the same
        order on the same data as ``rk4``.  One rank, fused path; a last shorter step runs through ``rk4``.
        ``sensors`` / ``monitor`` / ``receivers`` / ``energy`` / ``guard`` / ``record_from`` as in ``rk4``: their launches follow a replay
        on the same stream, outside the captured graph.  A solver with point sources cannot be replayed (their stage time is a launch argument; a device
        stage block for them does not exist yet): ``FusGpuError``.  Returns ``(t, steps)``."""
        if not self.fused or self.halo is not None:
            raise _lib.FusGpuError("rk4_graph: single-rank fused path only")
        for term in self._terms:
            if not term.capturable:
                raise _lib.FusGpuError(f"rk4_graph: {term.refusal}: use rk4")
        self._check_relaxation_step(dt)
        t, tf = float(start_time), float(final_time)
        rows, ends = [], []
        record = self._recording(t, tf, dt, max_steps, record_from, sensors, monitor, receivers, energy, guard)
        for t0, h in rk4_steps(t, tf, dt, max_steps):
            if h != dt:
                break
            rows.append([self._facet_source.stage_row(self._stage_time(t0, i, dt)) for i in range(4)])
            t = t0 + h
            ends.append(t)
        if rows:
            if not hasattr(self, "_graphs"):
                self._graphs = {}
                self._stage_slot = self._facet_source.stage_slot(self.tdt, self.dev)
            slot = self._stage_slot
            table = torch.from_numpy(np.asarray(rows, dtype=np.float64)).to(slot.dtype).to(self.dev)  # rounded on the host
            graph = self._step_graph(dt)
            self._fused_enter()
            for k in range(len(rows)):
                slot.copy_(table[k])
                graph.replay()
                for _ in record(ends[k]):  # one rank: no exchange, nothing yielded
                    pass
            self._fused_exit()
        steps = len(rows)
        if t < tf and (max_steps is None or steps < max_steps):
            t, more = self.rk4(t, tf, dt, None if max_steps is None else max_steps - steps, sensors, record_from, monitor, receivers, energy,
                               guard)
            steps += more
        return t, steps

    # -- the stiffness of the field by itself: the energy record (diagnostics.py) and the step bound below ---------------------------
    def _stiffness_of(self, x, y):
        """Generator: ``y += K(-1/rho) x`` with the operator this solver holds (``_stiffness_operator``: ``(operator, cell constants,
        what travels in its G position, dofmap)``), complete over the owned dofs; on a partitioned mesh through the halo schedule
        (forward exchange of ``x``, reverse exchange of ``y``), yielding where ``HaloApply`` yields.  Nothing of the solver's is written."""
        op, cc, G, dofmap = self._stiffness_operator()
        if self.halo is None:
            op(x, cc, y, G, dofmap)
        else:
            op = self.halo.concurrent_safe(op)
            yield from self.halo.schedule(lambda c_, G_, d_: op(x, c_, y, G_, d_), (cc, G, dofmap), [(self.halo.fwd, x)], [(self.halo.rev, y)])

    def _gather(self, values, reduce, seq):
        """Generator: every rank's ``values`` as an array [size, len(values)] (``bioheat.BioheatSpectral3D._gather``)."""
        if self.halo is None:
            return np.asarray([[float(v) for v in values]])
        if reduce is not None:
            reduce.put(seq, self.comm.rank, values)
            yield "reduce"
            return reduce.get(seq)
        from .scatterer import gather_floats

        every = gather_floats(self.comm, values)
        if len(every) != self.comm.size:  # the local row alone: no bootstrap spans the ranks
            raise _lib.FusGpuError(f"{type(self).__name__}: ranks driven from one process share no collective: pass "
                                   "reduce=InProcessGather(nranks) and drive the schedules in lock step")
        return every

    def _damping_rates(self, rates):
        """Generator: add to ``rates`` (fp64, local dofs, zero on entry) the diagonal damping rate of every owned dof: the absorbing
        facets' ``M_f2(1/(rho c)) 1 / M`` and ``2 sigma`` of a sponge layer.  Returns the largest ``sigma^2`` of this rank."""
        coef, detJ, fdm = self._absorbing_set
        diag = torch.zeros(self.ndofs, dtype=self.tdt, device=self.dev)
        if fdm.shape[0]:
            self.mass_facet(torch.ones_like(diag), coef, diag, detJ, fdm)  # coef = -1/(rho c): the sign of the stage's right-hand side
        if self.halo is not None:  # a facet dof may be another rank's: complete the owned entries
            wk = self.halo.rev.begin(diag)
            yield "reverse"
            self.halo.rev.end(diag, wk)
        n = self.nlocal
        rates[:n] -= diag[:n].to(torch.float64) / self._energy_mass()[:n].to(torch.float64)
        sigma2 = 0.0
        if self._sponge_term is not None:
            idx, sigma = self._sponge_term.built
            if len(idx):
                rates[torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(self.dev)] += torch.from_numpy(2.0 * np.asarray(sigma)).to(self.dev)
                sigma2 = float(np.max(np.asarray(sigma) ** 2))
        return sigma2

    def _diffusive_ratio(self):
        """The largest ``delta / c^2`` of this rank's medium (0: no diffusivity term in the equation)."""
        return 0.0

    def stable_time_step_schedule(self, safety=0.8, reduce=None, rtol=0.01, min_iterations=16, max_iterations=200):
        """Generator form of ``stable_time_step`` (yields where ``HaloApply`` yields, and after depositing partial sums in
        ``reduce``, an ``InProcessGather`` the ranks of one process share)."""
        from .reductions import Reducer
        from .stability import rk4_stable_step

        n, f64, red = self.nlocal, torch.float64, Reducer(self.dev)
        gen = torch.Generator().manual_seed(1234 + (self.comm.rank if self.halo is not None else 0))
        m = self._energy_mass()[:n].to(f64)
        x, y = (torch.zeros(self.ndofs, dtype=self.tdt, device=self.dev) for _ in range(2))
        v = (torch.rand(n, generator=gen, dtype=f64) - 0.5).to(self.dev)
        every = yield from self._gather(red.terms(sum0=(v, v, m)).tolist()[:1], reduce, 0)
        seq, vv = 1, float(every.sum())
        v, v_prev, beta = v / np.sqrt(vv), torch.zeros_like(v), 0.0
        alphas, betas, lam_prev, lam = [], [], None, None
        for it in range(max_iterations):
            x[:n] = v.to(self.tdt)
            y.zero_()
            yield from self._stiffness_of(x, y)  # y = -K x, complete over the owned dofs
            w = -y[:n].to(f64) / m - beta * v_prev  # minv K v - beta v_prev
            every = yield from self._gather(red.terms(sum0=(w, v, m)).tolist()[:1], reduce, seq)
            alpha = float(every.sum())
            w -= alpha * v
            every = yield from self._gather(red.terms(sum0=(w, w, m)).tolist()[:1], reduce, seq + 1)
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
        rates = torch.zeros(self.ndofs, dtype=f64, device=self.dev)
        sigma2 = yield from self._damping_rates(rates)
        dmax, bad = red.absmax(rates, n=n)
        if bad:
            raise _lib.FusGpuError(f"stable_time_step: {bad} damping rate(s) are not finite (a zero of the lumped mass?)")
        every = yield from self._gather([dmax, sigma2, self._diffusive_ratio()], reduce, seq)
        self.lambda_max = lam
        self.damping_max = float(every[:, 0].max()) + float(every[:, 2].max()) * lam
        self.stable_limit = rk4_stable_step(lam + float(every[:, 1].max()), self.damping_max)
        self._warned_step = False
        return safety * self.stable_limit

    def stable_time_step(self, safety=0.8):
        """``safety`` times the explicit RK4 step this mesh and medium admit, from the solver's own operators:

        ``lambda_max``    the largest Ritz value of the Lanczos recurrence for ``M^-1 K(1/rho)`` in the ``M`` inner product (``M``: the
                          lumped mass the stage divides by), its applies the solver's stiffness with its exchanges, its dot products
                          ``Reducer.terms`` on fp64 vectors; at least 16 applies, then until two successive values agree to 1 %.  Every
                          estimate is a lower bound of the eigenvalue.
        ``damping_max``   the largest diagonal damping rate over the owned dofs of every rank: the absorbing facets'
                          ``M_f2(1/(rho c)) 1 / M``, ``2 sigma`` of a sponge layer and, for Westervelt, ``max(delta / c^2) lambda_max``,
                          which bounds ``lambda_max(M^-1 K(delta / (rho c^2)))`` because the cell matrices are positive semi-definite.
        the limit         ``stability.rk4_stable_step(lambda_max + max sigma^2, damping_max)``: the largest ``dt`` for which the roots
                          of ``mu^2 + d mu + lambda = 0`` stay inside RK4's stability region for every stiffness and damping rate up
                          to the two bounds -- ``2 sqrt 2 / sqrt(lambda_max)`` without damping, ``2.785 / damping_max`` without
                          stiffness.  In between it is a model problem, not a proof: stiffness and damping do not commute, and the two
                          maxima belong to different dofs in general.

        ``lambda_max``, ``damping_max`` and the unscaled limit ``stable_limit`` stay on the solver; ``rk4`` with a longer ``dt`` warns
        once.  The nonlinear term of Westervelt, relaxation mechanisms and the source are not part of the bound.  On a partitioned mesh
        every rank calls this (``scatterer.gather_floats`` joins the sums); ranks driven from one process drive
        ``stable_time_step_schedule(safety, reduce=InProcessGather(nranks))`` in lock step."""
        dt = run_schedule(self.stable_time_step_schedule(safety))
        self.check_halo_health(f"{type(self).__name__}.stable_time_step")
        return dt

    # -- the solution on the host ------------------------------------------------------------------------------------------
    def u_sol(self, with_ghosts=False):
        """Owned part of the pressure field on the host; ``with_ghosts``: the whole local vector after a forward scatter
        (``scatter_fwd(u_n_d); u_n_d.copy_to_host(u_n)``, cuda/demo_linear_box.py:568-570 -- what point evaluation needs).
        Valid once ``rk4()`` has returned; mid-run, ``rk4(..., sensors=...)`` observes the field on the device."""
        if not with_ghosts:
            return self.u[: self.nlocal].detach().cpu().numpy()
        if self.halo is not None:
            self.halo.fwd(self.u)
            torch.cuda.synchronize()
            self.check_halo_health(f"{type(self).__name__}.u_sol(with_ghosts=True)")
        return self.u.detach().cpu().numpy()

    def v_sol(self):
        return self.v[: self.nlocal].detach().cpu().numpy()
