"""
``HaloApply``: the distributed operator apply  y += K x  on a partitioned mesh, its cell / row split and the schedules that
overlap the two halo exchanges with interior work (``scatterer.py`` has the exchanges and re-exports the class).
"""

from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .comm import NativeComm, as_comm
from .utils import compute_scatterer_data_flat, to_flat


class HaloApply:
    """Distributed operator apply  y += K x  on a partitioned mesh, with the
    halo exchange overlapped with interior-cell work (one process per GPU):

        fwd.begin(x) | apply(lead slice) apply(interior half 1) | fwd.end(x)
        apply(boundary cells)                               # the only cells touching ghost dofs
        rev.begin(y) | apply(lead slice) apply(interior half 2) | rev.end(y)

    This is the reference's per-stage sequence scatter_fwd -> stiffness ->
    scatter_rev (cuda/demo_linear_box.py:537-553) with its host syncs removed
    and the cells split so that both exchanges hide behind interior work.
    ``mesh.dofmap`` must list the ghost-touching cells first
    (``mesh.num_boundary_cells``), as ``BoxMesh`` does.

    Lead slices (``lead_cells``; profiles/r02z_overlap_*.log): the operator kernels hold every vector
    register of every CU (4 workgroups x 128 VGPRs per SIMD lane), and RCCL's send/recv kernel needs 264 per
    wave, so a kernel posted next to a chip-filling launch is not scheduled until that launch drains -- the
    exchange would run AFTER the interior cells, not under them.  Each overlapped region therefore starts
    with a launch too small to fill the chip (about 0.6 of the resident-workgroup slots): the exchange kernels
    become resident next to it and stay resident under the large launch that follows.
    """

    def __init__(self, mesh, op, comm, float_type, overlap=True, kernels=None, apply_fn=None, plan=None, lead_cells="auto",
                 schedule="auto"):
        from .scatterer import begin_all, scatter_forward, scatter_reverse  # (that module imports this one)

        self.mesh = mesh
        # the sub-launches of one apply run next to each other and next to the reverse exchange's receive kernel, all adding
        # into the same y: an operator with an atomic-free default (mass_operator) hands over its atomic twin
        self.op = getattr(op, "atomic", op)
        # ... unless the operator can be applied ROW BY ROW (``mass_operator``: y[d] depends on x[d] alone): the apply is then
        # split by dof instead of by cell -- set A: owned dofs the reverse exchange does not add into (one launch next to the
        # exchanges, all their entries, whatever cells those are in); set B: ghost dofs (their x arrives with the forward
        # exchange) and owned dofs that are ghosted elsewhere (the reverse receive adds into them), launched between the two
        # exchanges on the communicator's stream.  No launch and no receive kernel ever adds into the same y[d] concurrently,
        # so the atomic-free kernel stays valid at N > 1 (csrc/mass_gather.hpp).
        self._op_rows = op if hasattr(op, "apply_rows") and hasattr(op, "rows_available") else None
        self._row_sets = {}  # (dofmap pointer, vector length) -> uint8 marks or None (not available: cell split + atomics)
        comm = as_comm(comm)
        self.comm = comm
        # plan = (owners_data, ghosts_data) already computed (e.g. by the reference-style
        # compute_scatterer_data of a driver); default: exchange the indices over ``comm`` now
        od, gd = plan if plan is not None else compute_scatterer_data_flat(mesh.index_map, comm)
        self.owners_data, self.ghosts_data = od, gd
        self.fwd = scatter_forward(comm, od, gd, mesh.nlocal, float_type, kernels)
        self.rev = scatter_reverse(comm, od, gd, mesh.nlocal, float_type, kernels)
        self.overlap = overlap
        nb, nc = mesh.num_boundary_cells, mesh.ncells
        mid = nb + (nc - nb) // 2
        has_neighbours = (len(self.neighbour_ranks()) > 0)
        env = os.environ.get  # the switches of this class, all read here
        if schedule == "auto":
            schedule = env("FUS_HALO_SCHEDULE", "auto")
        self._lib_sync = env("FUS_HALO_EVENT_SYNC", "0") != "1"  # 1: fork / join the side stream with events
        self._fold_sync = env("FUS_HALO_FOLD_SYNC", "1") != "0"  # 0: fork / join as kernels of their own (A/B runs)
        self._attach_sync = env("FUS_HALO_ATTACH_SYNC", "1") != "0"  # 0: the fork's signal as a kernel of its own
        # "concurrent" (csrc/halo_ipc.hpp transports): ONE launch over all interior cells on the caller's stream; the
        # boundary cells and both exchanges on a high-priority side stream next to it (profiles/r03a_overlap_local.log:
        # a same-shape kernel on a second stream takes the workgroup slots the interior launch frees, so the apply is
        # not cut into three launches).  "split": interior half | boundary | interior half on one stream, the form
        # RCCL's kernel needs (with lead slices).
        if schedule == "auto":
            small_kernels = isinstance(comm, NativeComm) and comm.backend in ("peer", "peer-local", "local")
            schedule = "concurrent" if (small_kernels and apply_fn is None) else "split"
        if schedule not in ("concurrent", "split"):
            raise ValueError(f"schedule must be 'auto', 'concurrent' or 'split', got {schedule!r}")
        self.schedule_kind = schedule if overlap else "sequential"
        if schedule == "concurrent":
            lead_cells = 0  # lead slices exist for RCCL's kernel only
        if lead_cells == "auto":
            lead = self._auto_lead_cells(mesh)
            if (nc - nb) < 8 * lead:  # mesh too small to slice
                lead = 0
        else:
            lead = max(0, min(int(lead_cells or 0), mid - nb, nc - mid))
        if not overlap or not has_neighbours:  # nothing to hide
            lead = 0
        self.lead_cells = lead
        self.ranges = {"boundary": (0, nb), "lead1": (nb, nb + lead), "interior1": (nb + lead, mid),
                       "lead2": (mid, mid + lead), "interior2": (mid + lead, nc), "interior": (nb, nc)}
        self._events = None
        self._views_cache = {}
        self._apply_fn = apply_fn  # tests: CPU stand-in for the operator
        self._begin_all = begin_all
        self._warm = set()  # interior cell ranges (by the pointers of their per-cell arrays) that have been applied once
        self._hs = None

    @staticmethod
    def concurrent_safe(op):
        """The operator to use for anything that adds into the apply's output vector WHILE the apply runs -- the cell
        operator's sub-launches (done by ``HaloApply`` itself) and whatever a caller's ``boundary_terms`` launches: an operator
        with an atomic-free default (``mass_operator``: plain load + store per dof) hands over its float-atomic twin, every
        other operator is returned as it is."""
        return getattr(op, "atomic", op)

    def row_split(self, dofmap, ndofs):
        """The uint8 marks of the row split for ``dofmap`` on vectors of ``ndofs`` entries (0: set A, 1: set B), or ``None`` when
        the operator is not row-wise or its atomic-free kernel is not available for this dofmap (decided once per dofmap)."""
        if self._op_rows is None or self._apply_fn is not None or not isinstance(dofmap, torch.Tensor) or not dofmap.is_cuda:
            return None
        key = (dofmap.data_ptr(), int(ndofs), dofmap._version)
        if key not in self._row_sets:
            marks = torch.zeros(int(ndofs), dtype=torch.uint8, device=dofmap.device)
            marks[self.mesh.nlocal:] = 1
            ghosted = torch.from_numpy(np.ascontiguousarray(to_flat(self.ghosts_data)[0], dtype=np.int64)).to(dofmap.device)
            if ghosted.numel():
                marks[ghosted] = 1
            self._row_sets[key] = marks if self._op_rows.rows_available(dofmap, int(ndofs), marks) else None
        return self._row_sets[key]

    def neighbour_ranks(self):
        """Neighbour ranks of this rank (either direction)."""
        od, gd = self.owners_data, self.ghosts_data
        return [int(r) for r in list(np.asarray(od[-1]).reshape(-1)) + list(np.asarray(gd[-1]).reshape(-1))]

    @staticmethod
    def _auto_lead_cells(mesh):
        """Cells of a launch that fills about 0.6 of the chip's resident-workgroup slots (4 workgroups per
        CU up to P = 5, 3 above: tools/resource_usage.py)."""
        try:
            nd = int(mesh.dofmap.shape[1])
            P = int(round(nd ** (1.0 / 3.0))) - 1
            ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
            epb = int(_lib.load().fus_plan_entities_per_batch(nd))
        except Exception:
            return 0
        if epb < 1 or (P + 1) ** 3 != nd:
            return 0
        return int(0.6 * ncu * (4 if P <= 5 else 3)) * epb

    def _halo_stream(self):
        if self._hs is None:
            lib_stream = self.comm.stream() if isinstance(self.comm, NativeComm) and self.comm.backend != "rccl" else None
            # high priority: small kernels between big ones
            self._hs = lib_stream if lib_stream is not None else torch.cuda.Stream(priority=-1)
        return self._hs

    @staticmethod
    def _plans_ready(views):
        """The batch plans of the dofmaps among ``views`` (int32 [cells, dofs per cell]) are cached: the launch does no set-up."""
        from . import operators as ops

        dms = [t for t in views if t.dtype == torch.int32 and t.dim() == 2 and t.shape[1] > 8]
        return len(dms) > 0 and all(ops._PLANS.has(t) for t in dms)

    def _views(self, name, percell):
        key = (name,) + tuple(t.data_ptr() for t in percell)
        v = self._views_cache.get(key)
        if v is None:
            a, b = self.ranges[name]
            v = tuple(t[a:b] for t in percell)  # views are kept so the operators' plan cache hits
            self._views_cache[key] = v
        return v

    def run(self, cell_fn, percell, forward, reverse, boundary_terms=None):
        """Generic overlapped stage.  ``cell_fn(*views)`` applies the cell operator(s) to one
        contiguous sub-range of cells, given views of the per-cell tensors ``percell`` (constants,
        G, detJ, dofmap, ...).  ``forward`` / ``reverse``: lists of ``(scatter closure, vector)``.
        ``boundary_terms()`` adds boundary-facet contributions; it runs after every forward scatter
        has landed and before the reverse scatters are posted (facet dofs can be ghosts).  In the concurrent schedule it
        runs NEXT TO the interior launch: whatever it launches must add with atomics (``concurrent_safe(op)``)."""
        for _ in self.schedule(cell_fn, percell, forward, reverse, boundary_terms):
            pass

    # the cell sub-ranges of the single-stream stage: before the forward exchange is completed, between the two exchanges, and
    # after the reverse exchange is posted
    _SEQUENTIAL = ((), ("boundary", "lead1", "interior1", "lead2", "interior2"), ())
    _SPLIT = (("lead1", "interior1"), ("boundary",), ("lead2", "interior2"))

    def schedule(self, cell_fn, percell, forward, reverse, boundary_terms=None, by_rows=False):
        """``by_rows``: ``cell_fn(which)`` applies the operator to row set ``which`` (0: A, 1: B; see ``row_split``) over ALL cells;
        ``percell`` is unused.

        The stage of ``run`` as a generator that yields each time this rank has POSTED a set of
        exchanges (``"forward"`` / ``"reverse"``) and is about to do work that does not depend on
        them.  One rank per process never needs the yields (``run`` just exhausts them); a host
        that drives several ranks from one thread (``NativeComm(local=...)``) advances all ranks'
        generators in lock step, so every rank has posted before any rank completes."""
        begin_all = self._begin_all

        def part(name):
            if by_rows:  # set A where the schedule has its (first) interior launch, set B in place of the boundary cells
                if name in ("interior", "interior1"):
                    cell_fn(0)
                elif name == "boundary":
                    cell_fn(1)
                return
            a, b = self.ranges[name]
            if b > a:
                cell_fn(*self._views(name, percell))

        if self.overlap and by_rows and boundary_terms is not None:
            raise ValueError("a row-split apply takes no boundary_terms (they would add into rows of set A next to its launch)")
        if self.schedule_kind == "concurrent" and (by_rows or (len(percell) > 0 and percell[0].is_cuda)):
            # main stream: ONE launch over all interior cells.  Side stream (the communicator's own high-priority stream
            # where the library has one: send, receive and the boundary kernels then follow each other in stream order,
            # no event edge between them): forward exchange -> boundary cells -> reverse exchange.
            main, side = torch.cuda.current_stream(), self._halo_stream()
            # fork / join: the library's event-free pair where the side stream is the communicator's (2.4 us on the
            # caller's stream instead of 7 + 3.5 for event record / wait next to chip-filling launches); events otherwise
            lib_sync = side is getattr(self.comm, "_stream", None) and self._lib_sync
            if self._events is None:
                self._events = (torch.cuda.Event(), torch.cuda.Event())
            ev_start, ev_side = self._events
            # PEER: fork and join are folded into the first send / last receive kernel of the chain (two kernels fewer)
            fold = lib_sync and getattr(self.comm, "transport", None) == "peer" and self._fold_sync
            # ... and the fork's signal rides on the interior launch itself (planned kernels publish the fork flag when their
            # first workgroup starts).  The flag then depends on the HOST reaching that launch, so nothing that can
            # synchronise the device may sit between the fork and the launch: the launch follows the fork at once (the
            # forward exchange is posted after it; it still runs under the interior kernel), and only once this cell
            # range has been applied before -- its batch plan exists, no first-use set-up inside the launch call.
            a_, b_ = self.ranges["interior"]
            warm_key = ("interior",) + (() if by_rows else tuple(t.data_ptr() for t in percell))
            attach = (lib_sync and self._attach_sync and self._apply_fn is None and not by_rows and b_ > a_ and warm_key in self._warm
                      and self._plans_ready(self._views("interior", percell)))
            if lib_sync:
                self.comm.fork(lazy=fold and len(forward) > 0, attach=attach)
            else:
                ev_start.record(main)
                side.wait_event(ev_start)
            part("interior")
            if attach:
                self.comm.fork_flush()  # a launch that could not carry the signal (plan-free kernel): a signal kernel after all
            self._warm.add(warm_key)
            with torch.cuda.stream(side):
                fw = begin_all(forward)
            yield "forward"
            with torch.cuda.stream(side):
                for sc, vec, wk in fw:
                    sc.end(vec, wk)
                part("boundary")
                if boundary_terms is not None:
                    boundary_terms()
                rv = begin_all(reverse, arm_join=self.comm if (fold and len(reverse) > 0) else None)
            yield "reverse"
            with torch.cuda.stream(side):
                for sc, vec, wk in rv:
                    sc.end(vec, wk)
                if not lib_sync:
                    ev_side.record(side)
            if lib_sync:
                self.comm.join()
            else:
                main.wait_event(ev_side)
            return
        # One stream.  NativeComm: begin() hands pack -> exchange -> unpack to the library's own high-priority
        # stream and returns; end() only makes this stream wait for it.  TorchComm: pack is
        # enqueued here, the collective on RCCL's stream, the unpack in end().
        before, middle, after = self._SPLIT if self.overlap else self._SEQUENTIAL
        fw = begin_all(forward)
        yield "forward"
        for name in before:
            part(name)
        for sc, vec, wk in fw:
            sc.end(vec, wk)
        for name in middle:
            part(name)
        if boundary_terms is not None:
            boundary_terms()
        rv = begin_all(reverse)
        yield "reverse"
        for name in after:
            part(name)
        for sc, vec, wk in rv:
            sc.end(vec, wk)

    def apply(self, x, cell_constants, y, G, dofmap, extra_forward=(), boundary_terms=None):
        """y += K x on the partitioned mesh (``extra_forward``: further ``(scatter_forward closure,
        vector)`` pairs to refresh alongside x, e.g. v_n of the RK stage)."""
        for _ in self.apply_schedule(x, cell_constants, y, G, dofmap, extra_forward, boundary_terms):
            pass

    def apply_schedule(self, x, cell_constants, y, G, dofmap, extra_forward=(), boundary_terms=None):
        """``apply`` as a generator (see ``schedule``)."""
        cell_fn, percell, by_rows = self._cell_fn(x, cell_constants, y, G, dofmap, rows=boundary_terms is None)
        return self.schedule(cell_fn, percell, [(self.fwd, x)] + list(extra_forward), [(self.rev, y)], boundary_terms, by_rows=by_rows)

    def _cell_fn(self, x, cell_constants, y, G, dofmap, rows=True):
        """``(cell_fn, percell, by_rows)`` of ``schedule`` for  y += K x : the row split where the operator offers it (and ``rows``),
        the cell split otherwise."""
        marks = self.row_split(dofmap, min(x.numel(), y.numel())) if rows else None
        if marks is not None:
            op = self._op_rows
            return (lambda which: op.apply_rows(x, cell_constants, y, G, dofmap, marks, which)), (), True
        fn = self._apply_fn if self._apply_fn is not None else self.op
        return (lambda c_, G_, d_: fn(x, c_, y, G_, d_)), (cell_constants, G, dofmap), False

    def prepare(self, x, cell_constants, G, dofmap):
        """Set-up, not an apply: build the batch plans of the three cell sub-ranges and bring the
        communicator up (RCCL creates its channels on first use) with two no-effect exchanges --
        a forward scatter of x (ghosts receive their owners' values) and a reverse scatter of a
        zero vector."""
        if self.row_split(dofmap, x.numel()) is None:  # (a row-split apply has built its three transposed plans by now)
            for name in self._launch_names():
                a, b = self.ranges[name]
                if b > a and self.op is not None and hasattr(self.op, "prepare"):
                    self.op.prepare(self._views(name, (cell_constants, G, dofmap))[2])
        # the device-side waits of the PEER transport are bounded: line the ranks up on the host before the first
        # exchange, so that a rank whose set-up took longer is not mistaken for a dead one
        if hasattr(self.comm, "barrier") and not getattr(self.comm, "in_process", False):
            self.comm.barrier()
        self.fwd(x)
        self.rev(x.new_zeros(x.shape))

    def apply_local_only(self, x, cell_constants, y, G, dofmap):
        """The three kernel launches without any exchange (bench: kernel time at N > 1)."""
        cell_fn, percell, by_rows = self._cell_fn(x, cell_constants, y, G, dofmap)
        if by_rows:
            for which in (1, 0):
                cell_fn(which)
            return
        for name in self._launch_names():
            a, b = self.ranges[name]
            if b > a:
                cell_fn(*self._views(name, percell))

    def apply_no_exchange(self, x, cell_constants, y, G, dofmap):
        """The launches of ``apply`` in its own schedule (streams, events, sub-ranges) with NO exchange: what cutting
        the apply into sub-launches costs by itself (bench.py: ``halo_split_cost_ms``).  Not an apply."""
        cell_fn, percell, by_rows = self._cell_fn(x, cell_constants, y, G, dofmap)
        for _ in self.schedule(cell_fn, percell, [], [], None, by_rows=by_rows):
            pass

    def _launch_names(self):
        """The cell sub-ranges this schedule launches, in issue order."""
        if self.schedule_kind == "concurrent":
            return ("boundary", "interior")
        return ("lead1", "interior1", "boundary", "lead2", "interior2")

    def health(self):
        """Failed device-side waits (time-outs, poisoned flags of failed neighbours) of EVERY closure of this communicator
        and of its fork / join kernels (0 = every exchange so far delivered); synchronises the exchange streams."""
        if isinstance(self.comm, NativeComm) and self.comm.handle:
            return self.comm.health()
        return 0

    def check_health(self, what="halo exchange"):
        """Raise if any exchange of this communicator failed on this rank (a device-side wait gave up, or a neighbour's
        failure reached this rank through a poisoned flag).  The reference would block in MPI Waitall
        (cuda/scatterer.py:175); here every wait is bounded, so a failure must be made loud instead."""
        n = self.health()
        if n:
            d = self.comm.health_detail() if hasattr(self.comm, "health_detail") else {}
            raise _lib.FusGpuError(
                f"{what}: {n} device-side wait(s) of the halo exchange failed on rank {self.comm.rank} ({d.get('timeouts', '?')} time-out(s) after "
                f"FUS_IPC_SPIN_SECONDS, {d.get('poisoned', '?')} flag(s) poisoned by a neighbour's failed exchange, {d.get('sync_timeouts', '?')} "
                "fork / join time-out(s)): ghost data is stale, the result is INVALID")
