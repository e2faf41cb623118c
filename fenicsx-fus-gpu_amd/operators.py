"""
Operator call surface of the reference, over libfusgpu.so (hand-written HIP for
gfx950).  Both flavours of the reference are served by the same objects:

numba-cpu flavour (numba-cpu/operators.py):
    mass_operator(N, float_type)            -> op(x, entity_constants, y, entity_detJ, entity_dofmap)   :19-68
    stiffness_operator(P, dphi, float_type) -> op(x, cell_constants, y, G, dofmap)                      :71-227
    axpy(local_size)                        -> kernel(alpha, x, y)                                      :230-251
    copy(a, b); fill(alpha, x); pointwise_divide(a, b, c)                                               :254-300

cuda flavour (cuda/operators.py), launched as ``kernel[grid, block](args...)``:
    mass_operator[g, b](x, entity_constants, y, detJ_entity, entity_dofmap)                             :18-70
    stiffness_operator(P, float_type)       -> op[g, b](x, consts, y, G, dofmap, dphi)                  :73-192
    axpy[g, b](alpha, x, y); copy[g, b](a, b); fill[g, b](alpha, x);
    pointwise_divide[g, b](a, b, c); square[g, b](a, b)                                                 :195-274

The launch configuration given in ``[grid, block]`` is accepted and ignored: the
library chooses its own geometry for CDNA4.  Arrays are device arrays (torch
tensors on the GPU, e.g. from ``device.to_device``); ``y`` / outputs are
modified in place; launches are asynchronous on torch's current HIP stream.
Argument errors raise (TypeError / ValueError) like a numba dispatch failure;
there is no CPU fallback.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib

_req = _lib.require_device_tensor

# The stiffness operator builds a batch plan (csrc/plan.hpp) the first time it sees a dofmap and
# reuses it while that dofmap array is unchanged.  FUS_STIFFNESS_PLAN=0 (or use_plan(False))
# selects the plan-free kernel that reads ``dofmap`` directly.
_USE_PLAN = os.environ.get("FUS_STIFFNESS_PLAN", "1") != "0"


def use_plan(flag: bool):
    global _USE_PLAN
    _USE_PLAN = bool(flag)


# Set-up-time locality ordering of the plan's batches (FUS_PLAN_LOCALITY_ORDER=0 / use_locality_order(False)
# turns it off): when a dofmap's cells are not already sorted by their smallest dof, a second plan
# is built with the cells taken in that order (an index indirection inside the plan: G, detJ and the
# constants stay where they are) and kept if its batches touch fewer distinct dofs.  A mesh with
# consecutive cells adjacent (BoxMesh, a bandwidth-reordered dolfinx mesh) is left alone; a random cell
# order goes from 0.365 back to 0.243 ms per apply at P = 4, 10 M dofs (profiles/r02c_numbering.log).
_LOCALITY_ORDER = os.environ.get("FUS_PLAN_LOCALITY_ORDER", "1") != "0"
# Two-row strip order for the plans of the scatter-bound kernels (plan_tiles.py).  OFF by default -- a measured negative
# (profiles/r05d_geom_variance_probe.log, r05e_*): 2 x 5 pieces touch 8 % fewer distinct dofs than 10 cells in a row (94.8 against 102.9
# per cell at P = 4) but flush them in MORE 64-byte atomic requests (45 runs of 21 dofs instead of 25 runs of 41), and the request
# count is what bounds these kernels: 156 us against 153.5 us for the in-kernel-geometry kernel at config 3.
# FUS_PLAN_STRIP_ORDER=1 / use_strip_order(True) turns it on (experiments).
_STRIP_ORDER = os.environ.get("FUS_PLAN_STRIP_ORDER", "0") == "1"


def use_strip_order(flag: bool):
    global _STRIP_ORDER
    _STRIP_ORDER = bool(flag)


def use_locality_order(flag: bool):
    global _LOCALITY_ORDER
    _LOCALITY_ORDER = bool(flag)


_MASS_PLAN_MIN_ENTRIES = 1 << 15  # below this the plan-free kernel is already launch-bound

# The mass apply WITHOUT atomics (csrc/mass_gather.hpp): one thread per touched dof sums its (entity, local index) entries
# from the transposed dofmap.  FUS_MASS_GATHER=0 / use_mass_gather(False) keeps the atomic kernels everywhere.
_USE_GATHER = os.environ.get("FUS_MASS_GATHER", "1") != "0"
# mean entries per touched dof above which the gather loses to the atomic batch plan: at P = 2 (27 / 8 = 3.4 entries per dof,
# one-element detJ segments) 0.262 against 0.200 ms, at P = 3 (2.4) 0.142 against 0.158 (profiles/r04t_ab_mass_gather.log)
_GATHER_MAX_MEAN_ENTRIES = 2.6
# ... the STATIC-detJ form of the gather (detJ streamed in row order instead of gathered through one-element segments) wins up to P = 2:
# 0.135 against 0.176 ms fp64 (0.60 of the roofline instead of 0.46), 0.071 against 0.134 ms fp32, where the plain gather takes 0.242 / 0.139
# (profiles/r06g_ab_mass_low_degree.log).  P = 1 (8 entries per dof) stays on the atomic plan.
_GATHER_STATIC_MAX_MEAN_ENTRIES = 4.0


def use_mass_gather(flag: bool):
    global _USE_GATHER
    _USE_GATHER = bool(flag)


# ------------------------------------------------------------------------- caches
class _Cache:
    """What the three workspace caches below share.  A key names the identity of an array (pointer, shape, torch version counter);
    an entry is a tuple ``(workspace, that array, ...)`` -- it holds the array itself: while the entry is cached the array's memory
    cannot be freed and handed to another one with the same address / shape / version -- or ``None`` when the library refused to
    build one.  Bounded: a full cache drops (and releases) its oldest entry.  ``dependants``: the caches whose entries are built
    on this one's; they are cleared with it.  A subclass supplies the key and ``_build``."""

    _held = None  # while a hipGraph is captured: every (workspace, keyed array) any of the caches handed out

    def __init__(self, capacity, *dependants):
        self._entries, self.capacity, self._dependants = {}, capacity, dependants

    @staticmethod
    def start_recording():
        _Cache._held = []

    @staticmethod
    def stop_recording():
        """-> the (workspace, keyed array) tensors handed out since ``start_recording``: whoever baked their addresses
        into a captured graph holds this list, so eviction from a cache cannot free them."""
        held, _Cache._held = _Cache._held or [], None
        return held

    def _lookup(self, key, *build_args):
        hit = self._entries.get(key, self)  # (self: no entry -- None is one)
        if hit is self:
            hit = self._build(*build_args)
            if len(self._entries) >= self.capacity:
                self._release(self._entries.pop(next(iter(self._entries))))
            self._entries[key] = hit
        return hit

    @staticmethod
    def _hand_out(hit):
        if hit is not None and _Cache._held is not None:
            _Cache._held.append(hit[:2])
        return hit

    @staticmethod
    def _release(hit):
        if hit is not None:
            _lib.load().fus_plan_release(hit[0].data_ptr())

    def clear(self):
        for cache in self._dependants:
            cache.clear()
        for hit in self._entries.values():
            self._release(hit)
        self._entries.clear()


class _StaticDetJCache(_Cache):
    """Static companions of transposed-dofmap plans (``fus_mass_gather_static_*``): detJ in row order, keyed on the plan's
    workspace and on the identity of the detJ array.  An entry is ``None`` when the library refused (a block of 256 dofs
    spanning more than 65 535 entities)."""

    def get(self, plan_ws, detJ, n_per, nent):
        key = (plan_ws.data_ptr(), detJ.data_ptr(), tuple(detJ.shape), detJ._version, detJ.dtype)
        return self._hand_out(self._lookup(key, plan_ws, detJ, n_per, nent))

    def _build(self, plan_ws, detJ, n_per, nent):
        lib = _lib.load()
        nbytes = lib.fus_mass_gather_static_bytes(int(n_per), int(nent), detJ.element_size())
        if nbytes <= 0:
            return None
        sws = torch.empty(int(nbytes), dtype=torch.uint8, device=detJ.device)
        fn = getattr(lib, f"fus_mass_gather_static_build_{_lib.suffix(detJ.dtype)}")
        rc = fn(plan_ws.data_ptr(), detJ.data_ptr(), sws.data_ptr(), int(nbytes), _lib.stream_ptr())
        if rc == _lib.ERR_UNSUPPORTED_ENTITY:
            return None
        _lib.check(rc, "fus_mass_gather_static_build")
        return sws, detJ, plan_ws  # holds the plan too: its address cannot be re-used while this lives


class _GatherPlanCache(_Cache):
    """Transposed-dofmap plans of the atomic-free mass apply, keyed like the batch plans (identity of the dofmap array) plus
    the length of the dof vectors.  An entry is ``None`` when the library refused the dofmap (a dof with more than 255
    entries) or the gather would lose (``_GATHER_STATIC_MAX_MEAN_ENTRIES``): the caller then takes the atomic path.  Otherwise it is
    ``(workspace, dofmap, the four info integers, kept for the static-detJ form alone, row_set or None)``."""

    def get(self, dofmap: torch.Tensor, ndofs: int, rows=None, static=False):
        """``rows = (row_set, which)``: the plan of the dofs d with ``row_set[d] == which`` only (device uint8[ndofs]; the
        partitioned apply's split into rows next to the exchanges and rows between them).  ``static``: the caller will apply the
        static-detJ form, which pays up to a higher mean number of entries per dof than the plain gather."""
        nent, N = dofmap.shape
        key = (dofmap.data_ptr(), nent, N, dofmap._version, dofmap.device.index, int(ndofs))
        if rows is not None:
            row_set, which = rows
            _req(row_set, torch.uint8, "row_set")
            if row_set.numel() != int(ndofs):
                raise ValueError("row_set must have one mark per dof")
            key = key + (row_set.data_ptr(), row_set._version, int(which))
        hit = self._lookup(key, dofmap, int(ndofs), rows)
        if hit is None or (hit[3] and not static):
            return None  # (the plain gather would lose on this dofmap: the caller takes the atomic batch plan)
        return self._hand_out(hit)

    def _build(self, dofmap, ndofs, rows):
        lib = _lib.load()
        nent, N = dofmap.shape
        nbytes = lib.fus_mass_gather_plan_bytes(N, nent, ndofs)
        if nbytes <= 0:
            return None
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dofmap.device)
        if rows is None:
            rc = lib.fus_mass_gather_plan_build(dofmap.data_ptr(), N, nent, ndofs, ws.data_ptr(), int(nbytes), _lib.stream_ptr())
        else:
            rc = lib.fus_mass_gather_plan_build_rows(dofmap.data_ptr(), N, nent, ndofs, rows[0].data_ptr(), int(rows[1]),
                                                     ws.data_ptr(), int(nbytes), _lib.stream_ptr())
        if rc == _lib.ERR_UNSUPPORTED_ENTITY:
            return None
        _lib.check(rc, "fus_mass_gather_plan_build")
        info = (C.c_int64 * 4)()
        _lib.check(lib.fus_mass_gather_plan_info(ws.data_ptr(), info), "fus_mass_gather_plan_info")
        if rows is not None:  # (a row subset is judged by the full plan: the caller asks for it only when the full plan was kept)
            return ws, dofmap, tuple(int(v) for v in info), False, rows[0]
        if not (info[0] > 0 and nent * N <= _GATHER_STATIC_MAX_MEAN_ENTRIES * info[0]):
            lib.fus_plan_release(ws.data_ptr())
            return None
        return ws, dofmap, tuple(int(v) for v in info), nent * N > _GATHER_MAX_MEAN_ENTRIES * info[0], None


class _PlanCache(_Cache):
    """Batch-plan workspaces keyed on the identity of the dofmap array (pointer, shape, version).
    One cache for the whole module: the cell mass operator and the stiffness operator share a
    plan when they are given the same dofmap.  An entry is ``(workspace, dofmap, entities per batch)``."""

    def __init__(self, capacity, *dependants):
        super().__init__(capacity, *dependants)
        self._plans = self._entries
        self.last_order = None  # cell order of the plan built last (None: natural order)

    def get(self, dofmap: torch.Tensor, exclusive_ndofs=None, external_use=None, strips=False):
        """-> (workspace tensor, entities_per_batch).  ``strips``: the plan of a kernel bound by its scatter side (in-kernel
        geometry, affine cells): its cell order interleaves adjacent rows of cells (``plan_tiles.two_row_strip_order``: 2 x 5
        pieces instead of 10 cells in a row at P = 4, -8 % distinct dofs per batch) when that lowers the number of distinct dofs
        the batches touch -- a separate cache entry from the row-ordered plan of the same dofmap, which the general-G kernels keep.  ``exclusive_ndofs`` (length of the vectors the plan is applied to):
        the plan also carries EXCLUSIVE-DOF MARKS (``fus_plan_mark_exclusive``: a dof touched by exactly one batch is finished
        with a plain load + store instead of a float atomic), a separate cache entry from the unmarked plan of the same
        dofmap.  ``external_use``: device int32[ndofs], what else adds into each dof while a launch with this plan runs
        (default: nothing -- the launch runs alone or only next to launches of the same stream)."""
        nent, N = dofmap.shape
        strips = bool(strips) and _STRIP_ORDER and exclusive_ndofs is None
        key = (dofmap.data_ptr(), nent, N, dofmap._version, dofmap.device.index,
               None if exclusive_ndofs is None else (int(exclusive_ndofs), None if external_use is None else (external_use.data_ptr(), external_use._version)))
        if strips:
            key = key + ("strips",)
        ws, _, epb = self._hand_out(self._lookup(key, dofmap, exclusive_ndofs, external_use, strips))
        return ws, epb

    def _build(self, dofmap, exclusive_ndofs, external_use, strips):
        lib = _lib.load()
        nent, N = dofmap.shape
        epb = lib.fus_plan_entities_per_batch(N)
        if epb < 0:
            _lib.check(epb, "fus_plan_entities_per_batch")
        nbytes = lib.fus_plan_bytes(N, epb, nent)
        if nbytes < 0:
            _lib.check(int(nbytes), "fus_plan_bytes")

        def build(order):
            w = torch.empty(int(nbytes), dtype=torch.uint8, device=dofmap.device)
            _lib.check(
                lib.fus_plan_build_ordered(dofmap.data_ptr(), order.data_ptr() if order is not None else None, N, epb, nent,
                                           w.data_ptr(), int(nbytes), _lib.stream_ptr()),
                "fus_plan_build_ordered",
            )
            return w

        def distinct_dofs(w):  # sum over batches of the distinct dofs a batch touches
            nbatch = (nent + epb - 1) // epb
            return int((w[256:256 + 4 * nbatch].view(torch.int32) & 0xFFFF).sum().item())

        ws = build(None)
        self.last_order = None
        if _LOCALITY_ORDER and nent > 2 * epb:
            mins = dofmap.min(dim=1).values
            if not bool((mins[1:] >= mins[:-1]).all().item()):  # not already in that order
                order = torch.argsort(mins, stable=True).to(torch.int32)
                ws2 = build(order)
                if distinct_dofs(ws2) < 0.97 * distinct_dofs(ws):
                    ws, ws2, self.last_order = ws2, ws, order
                lib.fus_plan_release(ws2.data_ptr())  # the plan that was not kept
        if strips and nent > 4 * epb:
            n = int(round(N ** (1.0 / 3.0)))
            if n >= 3 and n**3 == N:  # cells of degree >= 2 in tensor-product local order
                from . import plan_tiles

                faces = torch.from_numpy(plan_tiles.face_interior_local_dofs(n)).to(dofmap.device)
                cand = plan_tiles.two_row_strip_order(dofmap[:, faces].cpu().numpy(),
                                                      None if self.last_order is None else self.last_order.cpu().numpy())
                if cand is not None:
                    order = torch.from_numpy(cand.astype("int32")).to(dofmap.device)
                    ws2 = build(order)
                    if distinct_dofs(ws2) < 0.97 * distinct_dofs(ws):
                        ws, ws2, self.last_order = ws2, ws, order
                    lib.fus_plan_release(ws2.data_ptr())
        if exclusive_ndofs is not None:
            use = (external_use.to(torch.int32).clone() if external_use is not None
                   else torch.zeros(int(exclusive_ndofs), dtype=torch.int32, device=dofmap.device))
            if use.numel() != int(exclusive_ndofs):
                raise ValueError("external_use must have one entry per dof")
            _lib.check(lib.fus_plan_mark_exclusive(ws.data_ptr(), N, epb, nent, use.data_ptr(), int(exclusive_ndofs), _lib.stream_ptr()),
                       "fus_plan_mark_exclusive")
            del use  # a temporary: the caching allocator hands its memory out again in stream order
        return ws, dofmap, epb

    def has(self, dofmap: torch.Tensor) -> bool:
        """True if an (unmarked) plan of ``dofmap`` is cached -- row-ordered or strip-ordered: an operator uses one of the two
        consistently, and ``HaloApply`` asks only for a cell range the operator has been applied to before -- so an apply with
        it does no set-up work (no allocation, no host synchronisation): what ``HaloApply`` needs to know before it lets a
        launch carry a fork signal."""
        nent, N = dofmap.shape
        key = (dofmap.data_ptr(), nent, N, dofmap._version, dofmap.device.index, None)
        return key in self._entries or key + ("strips",) in self._entries


# a clear takes what was built on the cleared entries with it: the transposed-dofmap plans of the mass apply go with the batch
# plans, the row-ordered detJ copies with the transposed plans
_STATIC_DETJ = _StaticDetJCache(8)
_GATHER_PLANS = _GatherPlanCache(16, _STATIC_DETJ)
_PLANS = _PlanCache(16, _GATHER_PLANS)


class _Launchable:
    """``obj[grid, block](...)`` == ``obj.launch(...)`` (launch config ignored)."""

    def __getitem__(self, launch_config):
        return self.launch


# --------------------------------------------------------------------------- mass
def _mass_gather_usable(nent, n_per):
    return _USE_GATHER and nent * n_per >= _MASS_PLAN_MIN_ENTRIES and n_per <= 2048 and nent * n_per < 2**31


def _mass_route(entity_dofmap, ndofs, atomic=False, static=False, entity_detJ=None):
    """Which kernel a mass apply takes, decided here alone: -> (route, workspaces) with the route one of ``_MASS_KERNELS`` (it
    completes the entry's name, ``fus_mass_apply_<route><type>``) and the workspace tensors that kernel reads in place of the dofmap
    (the batch plan is asked of ``_PLANS`` by the apply: it depends on the operator's exclusive-dof marks).  ``static``: an
    operator made with ``static_detJ=True``; without ``entity_detJ`` it is judged by the transposed plan alone."""
    nent, n_per = entity_dofmap.shape
    if not atomic and _mass_gather_usable(nent, n_per):
        plan = _GATHER_PLANS.get(entity_dofmap, ndofs, static=static)  # every dofmap value is checked against ndofs
        if plan is not None and static and entity_detJ is not None:
            companion = _STATIC_DETJ.get(plan[0], entity_detJ, n_per, nent)
            if companion is not None:
                return "gather_static_", (plan[0], companion[0])
            if plan[3]:  # no companion, and the plain gather would lose: the default path is the batch plan
                plan = None
        if plan is not None:
            return "gather_", (plan[0],)
    if _USE_PLAN and 2 <= n_per <= 4096 and nent * n_per >= _MASS_PLAN_MIN_ENTRIES:  # plan batches hold <= 4096 entries
        return "planned_", ()
    return "", ()


_MASS_KERNELS = {"gather_static_": "fus::mass_gather_kernel", "gather_": "fus::mass_gather_kernel", "planned_": "fus::mass_plan_kernel",
                 "": "fus::mass_kernel"}


def mass_kernel_name(entity_dofmap, ndofs, atomic=False, static=False):
    """Which kernel ``mass_operator``'s apply launches for this dofmap and vector length (bench.py reports it); ``static``: of an operator made
    with ``static_detJ=True`` (it keeps the gather kernel up to more entries per dof: P = 2)."""
    return _MASS_KERNELS[_mass_route(entity_dofmap, int(ndofs), atomic, bool(static))[0]]


def mass_rows_available(entity_dofmap, ndofs, row_set):
    """True if ``mass_operator``'s apply can run as two row-subset launches of the atomic-free kernel for this dofmap (the
    full transposed plan is one the operator would use, and both subsets build): what ``HaloApply`` asks before it splits a
    mass apply by dof instead of by cell.  Builds and caches the three plans."""
    nent, n_per = entity_dofmap.shape
    if nent == 0 or not _mass_gather_usable(nent, n_per):
        return False
    if _GATHER_PLANS.get(entity_dofmap, int(ndofs)) is None:
        return False
    return all(_GATHER_PLANS.get(entity_dofmap, int(ndofs), (row_set, w)) is not None for w in (0, 1))


def _mass_check(x, entity_constants, y, entity_detJ, entity_dofmap, N):
    """The argument check of every mass apply -> (dtype, number of entities, dofs per entity)."""
    dt = x.dtype if isinstance(x, torch.Tensor) else None
    for name, t in (("x", x), ("entity_constants", entity_constants), ("y", y), ("entity_detJ", entity_detJ)):
        _req(t, dt, name)
    _req(entity_dofmap, torch.int32, "entity_dofmap")
    if entity_dofmap.dim() != 2 or entity_detJ.shape != entity_dofmap.shape:
        raise ValueError("entity_dofmap must be [num_entities, N] and entity_detJ must have the same shape")
    nent, n_per = entity_dofmap.shape
    if N is not None and n_per != N:
        raise ValueError(f"operator was built for N={N} dofs per entity, dofmap has {n_per}")
    if entity_constants.numel() != nent:
        raise ValueError("entity_constants must have one value per entity")
    return dt, nent, n_per


def _mass_apply_rows(x, entity_constants, y, entity_detJ, entity_dofmap, row_set, which, N=None):
    """The rows ``row_set[d] == which`` of ``y += M(c) x`` with the atomic-free kernel (every row sums all its entries)."""
    dt, nent, n_per = _mass_check(x, entity_constants, y, entity_detJ, entity_dofmap, N)
    if nent == 0:
        return
    hit = _GATHER_PLANS.get(entity_dofmap, min(x.numel(), y.numel()), (row_set, int(which)))
    if hit is None:
        raise _lib.FusGpuError("no row-subset plan for this dofmap (mass_rows_available() says when there is one)")
    fn = getattr(_lib.load(), f"fus_mass_apply_gather_{_lib.suffix(dt)}")
    _lib.check(fn(x.data_ptr(), entity_constants.data_ptr(), y.data_ptr(), entity_detJ.data_ptr(), hit[0].data_ptr(), int(n_per), int(nent),
                  _lib.stream_ptr()), "fus_mass_apply_gather (row subset)")


def _mass_apply(x, entity_constants, y, entity_detJ, entity_dofmap, N=None, exclusive=False, atomic=False, static=False):
    dt, nent, n_per = _mass_check(x, entity_constants, y, entity_detJ, entity_dofmap, N)
    if nent == 0:
        return
    route, ws = _mass_route(entity_dofmap, min(x.numel(), y.numel()), atomic, static, entity_detJ)
    fn = getattr(_lib.load(), f"fus_mass_apply_{route}{_lib.suffix(dt)}")
    head = (x.data_ptr(), entity_constants.data_ptr(), y.data_ptr())
    if route == "gather_static_":  # detJ comes in row order from the companion
        rc = fn(*head, ws[0].data_ptr(), ws[1].data_ptr(), int(n_per), int(nent), _lib.stream_ptr())
    elif route == "planned_":
        plan, epb = _PLANS.get(entity_dofmap, exclusive_ndofs=y.numel() if exclusive else None)
        rc = fn(*head, entity_detJ.data_ptr(), plan.data_ptr(), int(n_per), int(epb), int(nent), _lib.stream_ptr())
    else:  # the transposed plan, or the dofmap itself
        rc = fn(*head, entity_detJ.data_ptr(), (ws[0] if ws else entity_dofmap).data_ptr(), int(n_per), int(nent), _lib.stream_ptr())
    _lib.check(rc, "fus_mass_apply_" + route + "*")


class _MassApply:
    """``operator(x, entity_constants, y, entity_detJ, entity_dofmap)`` returned by ``mass_operator(N, float_type)``;
    ``.atomic``: the same operator on the float-atomic kernels (safe next to concurrent writers of ``y``)."""

    def __init__(self, N, tdt, exclusive, atomic, static_detJ=False):
        self.N, self.dtype, self._exclusive, self._atomic, self._static = N, tdt, exclusive, atomic, bool(static_detJ) and not atomic
        self.atomic = self if atomic else _MassApply(N, tdt, exclusive, True)

    def __call__(self, x, entity_constants, y, entity_detJ, entity_dofmap):
        """``static_detJ=True``: the apply with detJ streamed in row order when this dofmap has a transposed plan and a static
        companion, the default path otherwise (same result)."""
        if isinstance(x, torch.Tensor) and x.dtype != self.dtype:
            raise TypeError(f"x: expected dtype {self.dtype}, got {x.dtype}")
        _mass_apply(x, entity_constants, y, entity_detJ, entity_dofmap, self.N, self._exclusive, self._atomic, self._static)

    def refresh(self):
        """``static_detJ=True``: forget the row-ordered copies of detJ.  REQUIRED after changing a detJ array in place through
        anything that writes through ``data_ptr()`` -- which includes THIS package's own vector ops (``fill`` / ``copy`` / ``axpy`` /
        ``pointwise_divide``) and every other C-ABI kernel (``compute_scaled_jacobian_determinant_device`` into the same array):
        they do not bump torch's version counter, the only change the cache notices by itself (torch's own in-place operations)."""
        _STATIC_DETJ.clear()

    def apply_rows(self, x, entity_constants, y, entity_detJ, entity_dofmap, row_set, which):
        """``y[d] += (M(c) x)[d]`` for the dofs with ``row_set[d] == which`` only (atomic-free kernel): the two halves of a
        partitioned apply (``HaloApply``), which never add into one ``y[d]`` concurrently."""
        if isinstance(x, torch.Tensor) and x.dtype != self.dtype:
            raise TypeError(f"x: expected dtype {self.dtype}, got {x.dtype}")
        _mass_apply_rows(x, entity_constants, y, entity_detJ, entity_dofmap, row_set, which, self.N)

    def rows_available(self, entity_dofmap, ndofs, row_set):
        return (not self._atomic) and mass_rows_available(entity_dofmap, ndofs, row_set)


class _MassOperator(_Launchable):
    def __call__(self, N: int, float_type, exclusive=False, atomic=False, static_detJ=False):
        """``mass_operator(N, float_type)`` -> ``operator(x, entity_constants, y, entity_detJ, entity_dofmap)``
        (numba-cpu/operators.py:19-68).

        Default kernel (csrc/mass_gather.hpp): ONE thread per touched dof sums the dof's (entity, local index) entries from
        the transposed dofmap in the order of the reference's serial loop and finishes ``y[dof]`` with a plain load +
        store -- no float atomics (their request rate bounds the atomic kernels at 0.44-0.45 of the HBM roofline), bitwise
        reproducible.  Like the reference's CPU operator (a plain ``+=``), such a launch assumes NOTHING ELSE adds into ``y``
        while it runs (earlier and later launches of the same stream are fine).  ``atomic=True`` (keyword, or the ``.atomic``
        attribute of the returned operator): the float-atomic kernels of cuda/operators.py:66-70's behaviour, safe next to
        another stream's launch or a halo receive adding into the same ``y`` -- what ``HaloApply`` uses for its overlapped
        sub-launches.  Dofmaps the gather does not pay for (P = 2: 3.4 entries per dof) or cannot hold (a dof in more than 255
        entities) take the atomic batch plan by themselves.
        ``exclusive=True`` (atomic batch plan with exclusive-dof marks, round 4's first attempt): kept for the atomic path,
        measured slower than the unmarked plan.
        ``static_detJ=True`` (opt-in): the caller declares ``entity_detJ`` constant across applies -- it is what the reference's
        drivers do (one detJ array for the whole run, cuda/demo_nonlinear_bowl.py:603-632) -- and the operator keeps a copy of it
        in ROW order next to the transposed dofmap: the kernel streams detJ instead of gathering it through the entry ids
        (bitwise the same result).  The copy is a SNAPSHOT: call ``op.refresh()`` after writing into detJ with anything but torch's
        own in-place operations -- this package's vector ops and device precompute write through ``data_ptr()`` and are NOT noticed.
        The constants are read per apply and may change."""
        return _MassApply(int(N), _lib.torch_dtype(float_type), exclusive, atomic, static_detJ)

    @staticmethod
    def launch(x, entity_constants, y, detJ_entity, entity_dofmap):
        _mass_apply(x, entity_constants, y, detJ_entity, entity_dofmap)


mass_operator = _MassOperator()


class DiagonalMassOperator:
    """The cell mass apply in CACHED-DIAGONAL form (opt-in; own bytes contract: 3 vector touches per dof).

    With GLL collocation the operator of numba-cpu/operators.py:19-68 is diagonal:  M(c) x = (M(c) 1) (.) x.
    ``DiagonalMassOperator(entity_constants, entity_detJ, entity_dofmap, ndofs)`` assembles ``w = M(c) 1`` once with the
    reference-compatible ``mass_operator`` (so ``w`` carries exactly its rounding) and ``op(x, y)`` then does
    ``y += w * x`` (``fus_muladd_*``).  The reference's drivers re-apply the gather / scatter form on every use
    (cuda/demo_nonlinear_bowl.py:603-632); the Westervelt solver of this package uses the same identity for its two
    mass terms.  ``w`` is valid for the (constants, detJ, dofmap) it was built from: ``refresh()`` after changing them.
    On a partitioned mesh ``w`` holds this rank's cells' contributions, like ``y`` after the cell operator (reverse-scatter
    either ``w`` once or ``y`` every time)."""

    def __init__(self, entity_constants, entity_detJ, entity_dofmap, ndofs, float_type=None):
        dt = entity_detJ.dtype if float_type is None else _lib.torch_dtype(float_type)
        _req(entity_constants, dt, "entity_constants")
        _req(entity_detJ, dt, "entity_detJ")
        _req(entity_dofmap, torch.int32, "entity_dofmap")
        self.dtype, self.ndofs = dt, int(ndofs)
        self._args = (entity_constants, entity_detJ, entity_dofmap)
        self.w = torch.zeros(self.ndofs, dtype=dt, device=entity_detJ.device)
        self._fn = getattr(_lib.load(), f"fus_muladd_{_lib.suffix(dt)}")
        self.refresh()

    def refresh(self):
        cc, detJ, dm = self._args
        self.w.zero_()
        _mass_apply(torch.ones(self.ndofs, dtype=self.dtype, device=self.w.device), cc, self.w, detJ, dm)

    def __call__(self, x, y):
        _req(x, self.dtype, "x")
        _req(y, self.dtype, "y")
        if x.numel() != self.ndofs or y.numel() != self.ndofs:
            raise ValueError(f"x and y must have {self.ndofs} entries")
        _lib.check(self._fn(self.w.data_ptr(), x.data_ptr(), y.data_ptr(), self.ndofs, _lib.stream_ptr()), "fus_muladd")


def diagonal_mass_operator(entity_constants, entity_detJ, entity_dofmap, ndofs, float_type=None):
    return DiagonalMassOperator(entity_constants, entity_detJ, entity_dofmap, ndofs, float_type)


def _ptrs(n, *tensors):
    """The pointer arguments of a facet set: null for an empty set (``n == 0``) and for a tensor that is not given."""
    return [t.data_ptr() if (n and t is not None) else None for t in tensors]


def _facet_field(dt, field, n_source):
    """Set B of the facet entry points, ``field = (x, c, detJ_f, facet_dofmap)`` or None, checked: -> (its four pointer
    arguments, its number of facets, the dofs per facet).  ``n_source``: the dofs per facet of a non-empty set A, else None."""
    if field is None:
        return [None] * 4, 0, n_source
    xB, cB, dB, dmB = field
    for name, t in (("x", xB), ("c", cB), ("detJ_field", dB)):
        _req(t, dt, name)
    _req(dmB, torch.int32, "field dofmap")
    nB = dmB.shape[0]
    if nB and (dB.shape != dmB.shape or cB.numel() != nB):
        raise ValueError("facet arrays: detJ must have the dofmap's shape, one constant per facet")
    if nB and n_source is not None and dmB.shape[1] != n_source:
        raise ValueError("both facet sets must have the same number of dofs per facet")
    return _ptrs(nB, *field), nB, (dmB.shape[1] if nB else 1) if n_source is None else n_source


def facet_terms(y, source, field, scalars=None):
    """The boundary-facet terms of one RK4 stage in one launch (csrc/mass.hpp, ``fus_facet_terms_*``):

        source = (c1, s1, c2, s2, detJ_f, facet_dofmap)   y += M_f(s1 c1 + s2 c2) 1      (c2 may be None)
        field  = (x, c, detJ_f, facet_dofmap)             y += M_f(c) x

    ``scalars``: device tensor holding (s1, s2) -- they are then read from device memory by the kernel
    (``fus_facet_terms_dev_*``; the s1, s2 of ``source`` are ignored), which is what lets a captured time
    step be replayed as a hipGraph with new source values.

    i.e. ``mass_operator(g, facet_coeff1, b, ...)`` [+ the dg term] and ``mass_operator(v_n, facet_coeff2, b, ...)``
    of cuda/demo_linear_box.py:546-549 / cuda/demo_nonlinear_bowl.py:633-641 without filling g into a vector."""
    c1, s1, c2, s2, dA, dmA = source
    dt = y.dtype if isinstance(y, torch.Tensor) else None
    _req(y, dt, "y")
    for name, t in (("c1", c1), ("detJ_source", dA)) + (() if c2 is None else (("c2", c2),)):
        _req(t, dt, name)
    _req(dmA, torch.int32, "source dofmap")
    nA = dmA.shape[0]
    if nA and (dA.shape != dmA.shape or c1.numel() != nA):
        raise ValueError("facet arrays: detJ must have the dofmap's shape, one constant per facet")
    pB, nB, N = _facet_field(dt, field, dmA.shape[1] if nA else None)
    if nA + nB == 0:
        return
    pc1, pc2, pdA, pdmA = _ptrs(nA, c1, c2, dA, dmA)
    if scalars is not None:
        _req(scalars, dt, "scalars")
        if scalars.numel() < 2:
            raise ValueError("scalars must hold (s1, s2)")
        fn = getattr(_lib.load(), f"fus_facet_terms_dev_{_lib.suffix(dt)}")
        _lib.check(fn(y.data_ptr(), pc1, pc2, scalars.data_ptr(), pdA, pdmA, int(nA), *pB, int(nB), int(N), _lib.stream_ptr()),
                   "fus_facet_terms_dev")
        return
    fn = getattr(_lib.load(), f"fus_facet_terms_{_lib.suffix(dt)}")
    _lib.check(fn(y.data_ptr(), pc1, float(s1), pc2, float(s2), pdA, pdmA, int(nA), *pB, int(nB), int(N), _lib.stream_ptr()),
               "fus_facet_terms")


def facet_source_terms(y, bound_array, field, stage=None, stage_dev=None):
    """``facet_terms`` with a phased-array source (csrc/source_array.hpp, ``fus_facet_source_array_*``):

        bound_array  a ``sources.BoundSourceArray``: per source facet its element and the set-A tensors (c1, c2, detJ, dofmap)
                     y += M_f(g_e c1 + dg_e c2) 1,  g_e / dg_e the value of each facet's element at the stage time
        field        (x, c, detJ_f, facet_dofmap) or None      y += M_f(c) x  (the absorbing term; None: no set B)

    The stage block ``{t, w0, A, f0, alpha, D}`` (fp64) is ``stage`` (host, ``bound_array.stage_scalars(t)``: copied into
    the launch) or ``stage_dev`` (a float64 device tensor read by the kernel, ``fus_facet_source_array_dev_*``: a captured
    hipGraph replays with new stage times).  Exactly one of them is given.

    A bound array that carries a sampled waveform (``bound_array.table``, sources.SampledWaveform) takes the table route
    (csrc/source_wave.hpp, ``fus_facet_source_wave_*``): ``g_e = a_e A w_r(t - tau_e)`` with ``r = row_of_element[e]``, interpolated
    in the kernel; same stage block (only ``t`` and ``A`` are read), same ``stage`` / ``stage_dev``."""
    ba = bound_array
    dt = y.dtype if isinstance(y, torch.Tensor) else None
    _req(y, dt, "y")
    if ba.dtype != dt:
        raise TypeError(f"the source array was bound for {ba.dtype}, y is {dt}")
    nA = ba.nfacets
    if nA:
        for name, t in (("coeff1", ba.coeff1), ("detJ_source", ba.detJ)) + (() if ba.coeff2 is None else (("coeff2", ba.coeff2),)):
            _req(t, dt, name)
        _req(ba.dofmap, torch.int32, "source dofmap")
        _req(ba.element_of_facet, torch.int32, "element_of_facet")
        for name, t in (("amplitude", ba.amplitude), ("phase", ba.phase), ("delay", ba.delay)):
            _req(t, torch.float64, name)
        if ba.detJ.shape != ba.dofmap.shape or ba.coeff1.numel() != nA or ba.dofmap.shape[0] != nA:
            raise ValueError("source facet arrays: detJ must have the dofmap's shape, one constant and one element id per facet")
    wave = getattr(ba, "table", None) is not None
    if wave:
        wave_args = _wave_table(ba, ba.array.waveform, ba.table, ba.row_of_element, ba.n_elements, y.device, "row_of_element")
    pB, nB, N = _facet_field(dt, field, ba.dofmap.shape[1] if nA else None)
    if nA + nB == 0:
        return
    if (stage is None) == (stage_dev is None):
        raise ValueError("facet_source_terms: give exactly one of stage (host) and stage_dev (device)")
    args = [y.data_ptr(), *_ptrs(nA, ba.coeff1, ba.coeff2, ba.detJ, ba.dofmap, ba.element_of_facet), int(nA)]
    if wave:
        args += [*_ptrs(nA, ba.amplitude, ba.delay, ba.row_of_element), int(ba.n_elements), *wave_args, *pB, int(nB), int(N)]
        family = "fus_facet_source_wave"
    else:
        args += [*_ptrs(nA, ba.amplitude, ba.phase, ba.delay), int(ba.n_elements), *pB, int(nB), int(N)]
        family = "fus_facet_source_array"
    if stage_dev is not None:
        _req(stage_dev, torch.float64, "stage_dev")
        if stage_dev.numel() < 6:
            raise ValueError("stage_dev must hold {t, w0, A, f0, alpha, D}")
        fn = getattr(_lib.load(), f"{family}_dev_{_lib.suffix(dt)}")
        _lib.check(fn(*args, stage_dev.data_ptr(), _lib.stream_ptr()), f"{family}_dev")
        return
    st = np.ascontiguousarray(np.asarray(stage, dtype=np.float64).reshape(-1))
    if st.size < 6:
        raise ValueError("stage must hold {t, w0, A, f0, alpha, D}")
    fn = getattr(_lib.load(), f"{family}_{_lib.suffix(dt)}")
    _lib.check(fn(*args, st.ctypes.data, _lib.stream_ptr()), family)


def _wave_table(holder, wf, table, row_of, n, device, name):
    """The table arguments ``(table, R, Nt, t0, dt)`` of the sampled-waveform entry points (csrc/source_wave.hpp), checked: ``table``
    fp64 ``[R, Nt, 2]`` with the ``Nt`` of the waveform ``wf``, 16-byte aligned, ``row_of`` int32 ``[n]`` with entries in ``[-1, R)``, both
    on ``device``.  The launch is launch-bound and runs four times per step, so the bound object ``holder`` remembers the two tensors
    it was checked with: the checks (the range check reads the map back) run again only when one of them is replaced."""
    seen = holder.__dict__.get("_wave_checked")
    if seen is not None and seen[0] is table and seen[1] is row_of and seen[2] == device:
        return seen[3]
    _req(table, torch.float64, "waveform table")
    _req(row_of, torch.int32, name)
    if table.dim() != 3 or table.shape[0] < 1 or table.shape[1] != wf.n_samples or table.shape[1] < 2 or table.shape[2] != 2:
        raise ValueError(f"waveform table: [R, {wf.n_samples}, 2] (value and derivative interleaved), got {tuple(table.shape)}")
    if row_of.shape != (n,):
        raise ValueError(f"{name}: one row per entry ({n}), got shape {tuple(row_of.shape)}")
    if table.device != device or row_of.device != device:
        raise ValueError("the waveform table and its row map must be on y's device")
    if table.data_ptr() % 16:
        raise ValueError("waveform table: must be 16-byte aligned")
    R = int(table.shape[0])
    args = [table.data_ptr(), R, int(table.shape[1]), float(wf.t0), float(wf.dt)]
    # (while a graph is captured the read-back would end the capture: the range is then checked by the next launch outside one; the
    # kernel skips a row outside [0, R) in any case)
    if not torch.cuda.is_current_stream_capturing():
        if n and (int(row_of.min()) < -1 or int(row_of.max()) >= R):
            raise ValueError(f"{name}: rows must lie in [-1, {R})")
        holder._wave_checked = (table, row_of, device, args)
    return args


def sponge_terms(y, u, v, bound):
    """The sponge layer's damping terms of one RK4 stage in one launch over the layer's dofs (csrc/sponge.hpp,
    ``fus_sponge_terms_*``): with ``bound = (idx, cu, cv)`` of ``sponge.SpongeLayer.bind``,

        y[idx] -= cv v[idx] + cu u[idx]

    ``(u, v)`` the stage's inputs, ``y`` its right-hand side.  The adds are float atomics (next to a halo the launch runs while
    the interior cells add into the same y).  An empty list is a no-op."""
    idx, cu, cv = bound
    dt = y.dtype if isinstance(y, torch.Tensor) else None
    for name, t in (("y", y), ("u", u), ("v", v), ("cu", cu), ("cv", cv)):
        _req(t, dt, name)
    _req(idx, torch.int32, "idx")
    n = idx.numel()
    if cu.numel() != n or cv.numel() != n:
        raise ValueError("sponge_terms: one cu and one cv per list entry")
    if u.numel() != y.numel() or v.numel() != y.numel():
        raise ValueError("sponge_terms: y, u and v must have the same number of entries")
    if any(t.device != y.device for t in (u, v, idx, cu, cv)):
        raise ValueError("sponge_terms: every operand must be on y's device")
    if n == 0:
        return
    fn = getattr(_lib.load(), f"fus_sponge_terms_{_lib.suffix(dt)}")
    _lib.check(fn(y.data_ptr(), u.data_ptr(), v.data_ptr(), idx.data_ptr(), cu.data_ptr(), cv.data_ptr(), int(n), _lib.stream_ptr()),
               "fus_sponge_terms")


RELAX_FIRST, RELAX_MIDDLE, RELAX_LAST = 0, 1, 2  # csrc/relax_table.hpp


def relax_stage(bw, aw, aw_u, kind, tau, kappa, xi0, xin, acc, u_base, vn, ur, nlocal):
    """The relaxation mechanisms' pass of one RK4 stage in one streaming launch (csrc/relaxation.hpp, ``fus_relax_stage_*``): per owned
    dof and mechanism, with ``k = kappa vn - xin / tau`` of the stage's inputs,

        FIRST   acc = xi0 + bw k ; xin = xi0 + aw k      MIDDLE   acc += bw k ; xin = xi0 + aw k      LAST   xi0 = acc + bw k

    and ``ur = (u_base + aw_u vn) + sum`` of the variables the next stage sees.  ``tau``: host array [NR] (fp64); ``kappa``: a host
    array [NR] (one scalar weight per mechanism: no weight vector is read) or a device tensor [NR, stride]; ``xi0`` / ``xin`` /
    ``acc``: device tensors [NR, stride], stride >= nlocal; ``u_base`` / ``vn`` / ``ur``: at least ``nlocal`` entries."""
    dt = xi0.dtype if isinstance(xi0, torch.Tensor) else None
    for name, t in (("xi0", xi0), ("xin", xin), ("acc", acc), ("u_base", u_base), ("vn", vn), ("ur", ur)):
        _req(t, dt, name)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    nr = tau.size
    if tau.ndim != 1 or not 1 <= nr <= 4 or xi0.ndim != 2 or xi0.shape[0] != nr or xin.shape != xi0.shape or acc.shape != xi0.shape:
        raise ValueError("relax_stage: 1 to 4 relaxation times, and xi0, xin, acc of one shape [NR, stride]")
    stride, nlocal = int(xi0.shape[1]), int(nlocal)
    if not 0 <= nlocal <= stride or min(u_base.numel(), vn.numel(), ur.numel()) < nlocal:
        raise ValueError("relax_stage: 0 <= nlocal <= stride, and u_base, vn, ur of at least nlocal entries")
    if isinstance(kappa, torch.Tensor):
        _req(kappa, dt, "kappa")
        if kappa.shape != xi0.shape:
            raise ValueError("relax_stage: per-dof weights have the shape of the state, [NR, stride]")
        ks, kd = None, kappa.data_ptr()
    else:
        ks = np.ascontiguousarray(kappa, dtype=np.float64)
        if ks.shape != (nr,):
            raise ValueError("relax_stage: one scalar weight per mechanism")
        kd = None
    if any(t.device != xi0.device for t in (xin, acc, u_base, vn, ur) + ((kappa,) if ks is None else ())):
        raise ValueError("relax_stage: every operand must be on xi0's device")
    if int(kind) not in (RELAX_FIRST, RELAX_MIDDLE, RELAX_LAST):
        raise ValueError(f"relax_stage: kind 0 (FIRST), 1 (MIDDLE) or 2 (LAST), got {kind}")
    fn = getattr(_lib.load(), f"fus_relax_stage_{_lib.suffix(dt)}")
    _lib.check(fn(float(bw), float(aw), float(aw_u), int(kind), nr, tau.ctypes.data, None if ks is None else ks.ctypes.data, kd,
                  xi0.data_ptr(), xin.data_ptr(), acc.data_ptr(), stride, u_base.data_ptr(), vn.data_ptr(), ur.data_ptr(), nlocal,
                  _lib.stream_ptr()), "fus_relax_stage")


def point_source_terms(y, bound, stage):
    """The point sources' terms of one RK4 stage in one launch (csrc/point_source.hpp, ``fus_point_source_*``): with ``bound`` a
    ``sources.BoundPointSources`` (the probe's tables ``cells`` / ``rows`` / ``weights`` and per-point ``amplitude`` / ``phase`` /
    ``delay``) and ``stage`` the host fp64 block ``{t, w0, A, f0, alpha, D}`` (``bound.stage_scalars(t)``),

        y[rows[cells[p]][ijk]] += g_p(t) Lx[i] Ly[j] Lz[k]

    ``y`` is the stage's right-hand side.  The adds are float atomics (points may share dofs; next to a halo the launch runs while
    the interior cells add into the same y).  No points is a no-op.

    Bound point sources that carry a sampled waveform (``bound.table``) take the table route (csrc/source_wave.hpp,
    ``fus_point_source_wave_*``): ``g_p = a_p A w_r(t - tau_p)`` with ``r = row_of_point[p]``."""
    bp = bound
    dt = y.dtype if isinstance(y, torch.Tensor) else None
    _req(y, dt, "y")
    if bp.dtype != dt:
        raise TypeError(f"the point sources were bound for {bp.dtype}, y is {dt}")
    _req(bp.weights, dt, "weights")
    _req(bp.cells, torch.int32, "cells")
    _req(bp.rows, torch.int32, "rows")
    for name, t in (("amplitude", bp.amplitude), ("phase", bp.phase), ("delay", bp.delay)):
        _req(t, torch.float64, name)
    m, n = bp.cells.numel(), bp.P + 1
    if bp.weights.numel() != m * 3 * n or any(t.numel() != m for t in (bp.amplitude, bp.phase, bp.delay)):
        raise ValueError("point_source_terms: weights [m, 3, P + 1] and one amplitude, phase and delay per point")
    if bp.rows.dim() != 2 or bp.rows.shape[1] != n**3:
        raise ValueError(f"point_source_terms: rows must be [k, {n**3}] dofmap rows")
    if y.numel() < bp.ndofs:
        raise ValueError(f"point_source_terms: y has {y.numel()} entries, the dofmap rows were checked against {bp.ndofs}")
    if any(t.device != y.device for t in (bp.weights, bp.cells, bp.rows, bp.amplitude, bp.phase, bp.delay)):
        raise ValueError("point_source_terms: every operand must be on y's device")
    wave = getattr(bp, "table", None) is not None
    if wave:
        wave_args = _wave_table(bp, bp.sources.waveform, bp.table, bp.row_of_point, m, y.device, "row_of_point")
    if m == 0:
        return
    st = np.ascontiguousarray(np.asarray(stage, dtype=np.float64).reshape(-1))
    if st.size < 6:
        raise ValueError("stage must hold {t, w0, A, f0, alpha, D}")
    if wave:
        fn = getattr(_lib.load(), f"fus_point_source_wave_{_lib.suffix(dt)}")
        _lib.check(fn(y.data_ptr(), bp.cells.data_ptr(), int(m), bp.rows.data_ptr(), int(bp.rows.shape[0]), bp.weights.data_ptr(),
                      int(bp.P), bp.amplitude.data_ptr(), bp.delay.data_ptr(), bp.row_of_point.data_ptr(), *wave_args, st.ctypes.data,
                      _lib.stream_ptr()), "fus_point_source_wave")
        return
    fn = getattr(_lib.load(), f"fus_point_source_{_lib.suffix(dt)}")
    _lib.check(fn(y.data_ptr(), bp.cells.data_ptr(), int(m), bp.rows.data_ptr(), int(bp.rows.shape[0]), bp.weights.data_ptr(), int(bp.P),
                  bp.amplitude.data_ptr(), bp.phase.data_ptr(), bp.delay.data_ptr(), st.ctypes.data, _lib.stream_ptr()),
               "fus_point_source")


def element_receive(u, dof, wgt, offsets, rec=None, slot=0, hre=None, him=None, coef=None):
    """The surface integrals of ``u`` over the elements of a receiving array in one launch (csrc/element_receive.hpp,
    ``fus_element_receive_*``): ``S_e = sum wgt[k] u[dof[k]]`` over ``k in [offsets[e], offsets[e + 1])``, written to row ``slot`` of
    ``rec`` [capacity, E] and accumulated into ``hre`` / ``him`` [H, E] with this step's factors ``coef`` [2H] (each optional).
    ``receivers.ElementReceivers`` builds the lists.  Summed in double in a fixed order, no atomics; no elements is a no-op."""
    dt = u.dtype if isinstance(u, torch.Tensor) else None
    _req(u, dt, "u")
    _req(wgt, dt, "wgt")
    _req(dof, torch.int32, "dof")
    _req(offsets, torch.int64, "offsets")
    E = offsets.numel() - 1
    if E < 0 or dof.numel() != wgt.numel():
        raise ValueError("element_receive: offsets [E + 1], one weight per dof entry")
    capacity = 0
    if rec is not None:
        _req(rec, dt, "rec")
        if rec.dim() != 2 or rec.shape[1] != E or not 0 <= int(slot) < rec.shape[0]:
            raise ValueError(f"element_receive: rec must be [capacity, {E}] with slot in [0, capacity)")
        capacity = rec.shape[0]
    H = 0
    if hre is not None or him is not None or coef is not None:
        for name, t in (("hre", hre), ("him", him), ("coef", coef)):
            _req(t, torch.float64, name)
        H = coef.numel() // 2
        if H < 1 or hre.shape != (H, E) or him.shape != (H, E):
            raise ValueError("element_receive: hre and him [H, E], coef [2H], H >= 1")
    if any(t is not None and t.device != u.device for t in (dof, wgt, offsets, rec, hre, him, coef)):
        raise ValueError("element_receive: every operand must be on u's device")
    if E == 0:
        return
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    fn = getattr(_lib.load(), f"fus_element_receive_{_lib.suffix(dt)}")
    _lib.check(fn(u.data_ptr(), ptr(dof), ptr(wgt), offsets.data_ptr(), int(E), ptr(rec), int(capacity), int(slot), ptr(hre), ptr(him),
                  ptr(coef), int(H), _lib.stream_ptr()), "fus_element_receive")


# ----------------------------------------------------------------- cell operators
def _to_device(a, dtype):
    """Host array or tensor -> contiguous tensor of ``dtype`` on the current device."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    return t.to(device=torch.device("cuda", torch.cuda.current_device()), dtype=dtype).contiguous()


class _CellOperator:
    """What the operators over the cells of a degree-P tensor-product mesh share: degree, type, the 1-D derivative table,
    the vertex geometry of the in-kernel-geometry kernels, and the argument checks of an apply."""

    def __init__(self, P, float_type, dphi=None):
        self.P = int(P)
        if not (_lib.MIN_DEGREE <= self.P <= _lib.MAX_DEGREE):
            raise ValueError(f"polynomial degree {P} outside the supported range {_lib.MIN_DEGREE}..{_lib.MAX_DEGREE}")
        self.n = self.P + 1
        self.dtype = _lib.torch_dtype(float_type)
        self._dphi = None if dphi is None else self._table(dphi)

    def _entry(self, name):
        return getattr(_lib.load(), f"fus_{name}_{_lib.suffix(self.dtype)}")

    def _table(self, dphi):
        """Accept the flat ``[q*n+i]`` (numba-cpu) or 2-D ``[q, i]`` (cuda) table, host or device."""
        if (dphi.numel() if isinstance(dphi, torch.Tensor) else np.size(dphi)) != self.n * self.n:
            raise ValueError(f"dphi must have {self.n * self.n} entries for P={self.P}")
        return _to_device(dphi, self.dtype).reshape(-1)

    def _geometry(self, x_g, pts, wts):
        """-> (x_g T[nvert, 3], pts T[n], wts T[n]) on the device: the vertices and the 1-D GLL rule G is formed from in the kernel."""
        xg, pt, wt = _to_device(x_g, self.dtype), _to_device(pts, self.dtype).reshape(-1), _to_device(wts, self.dtype).reshape(-1)
        if xg.dim() != 2 or xg.shape[1] != 3:
            raise ValueError("geometry: x_g must be [nvert, 3] (P1 hexahedra)")
        if pt.numel() != self.n or wt.numel() != self.n:
            raise ValueError(f"geometry: pts / wts must hold the {self.n} 1-D GLL points / weights")
        return xg, pt, wt

    def _check(self, dofmap, constants, tensors):
        """The argument check of every apply; ``constants`` and ``tensors`` are (name, tensor) pairs: all of them have the
        operator's type, ``dofmap`` is int32 [ncell, n^3], each of ``constants`` has one value per cell.  -> (ncell, n^3)"""
        for name, t in tensors + constants:
            _req(t, self.dtype, name)
        _req(dofmap, torch.int32, "dofmap")
        nd = self.n**3
        if dofmap.dim() != 2 or dofmap.shape[1] != nd:
            raise ValueError(f"dofmap must be [ncell, {nd}] for P={self.P}")
        ncell = dofmap.shape[0]
        for name, t in constants:
            if t.numel() != ncell:
                raise ValueError(f"{name} must have one value per cell")
        return ncell, nd

    def _check_G(self, G, ncell, nd):
        _req(G, self.dtype, "G")
        if G.numel() != ncell * nd * 6:
            raise ValueError(f"G must be [ncell, {nd}, 6]")

    @staticmethod
    def _check_x_dofs(x_dofs, ncell):
        _req(x_dofs, torch.int32, "x_dofs")
        if x_dofs.dim() != 2 or x_dofs.shape[1] != 8:
            raise ValueError("x_dofs must be [ncell, 8] (P1 hexahedra)")
        if ncell is not None and x_dofs.shape[0] != ncell:
            raise ValueError(f"geometry: x_dofs has {x_dofs.shape[0]} cells, dofmap has {ncell}")
        return x_dofs


class _StiffnessOperator(_CellOperator, _Launchable):
    """Returned by ``stiffness_operator``; callable both ways."""

    def __init__(self, P: int, float_type, dphi=None, affine_weights=None, geometry=None, nodal=None):
        if nodal is not None and geometry is None:  # (before anything is put on a device)
            raise ValueError("stiffness_operator(nodal=...) needs geometry=(x_dofs, x_g, pts, wts): the nodal kernel forms G from the "
                             "cell vertices.  For the general-G kernels scale the array once, nodal_medium.scale_G(G, kappa, dofmap), "
                             "and apply the plain operator to it")
        super().__init__(P, float_type, dphi)
        self._fn =self._entry("stiffness_apply")
        self._fn_planned = self._entry("stiffness_apply_planned")
        self._dphi_src = None
        # opt-in affine-cell fast path: tensor quadrature weights [n^3] of the rule G was built with
        self._wratio = None
        if affine_weights is not None:
            w = np.asarray(affine_weights, dtype=np.float64).reshape(-1)
            if w.size != self.n**3:
                raise ValueError(f"affine_weights must hold the {self.n ** 3} tensor quadrature weights")
            self._wratio = _to_device(w / w[0], self.dtype)
            self._fn_affine = self._entry("stiffness_apply_planned_affine")
        # opt-in in-kernel geometry: (x_dofs int32[ncell, 8], x_g T[nvert, 3], pts T[n], wts T[n]);
        # the G argument of the apply is then ignored (may be None)
        self._geom = None
        if geometry is not None:
            self._geom = (self._check_x_dofs(_to_device(geometry[0], torch.int32), None),) + self._geometry(*geometry[1:])
            self._fn_geom = self._entry("stiffness_apply_planned_geom")
        # opt-in nodal coefficient (in-kernel geometry only): kappa in the dof numbering of x, held by the operator, so that the call
        # surface stays op(x, cell_constants, y, G, dofmap) -- cell_constants a further factor per cell -- and a cell sub-range of a
        # halo schedule, which slices the per-cell tensors and passes x whole, needs nothing new
        self.nodal = None
        if nodal is not None:
            self.nodal = _to_device(nodal, self.dtype).reshape(-1)
            self._fn_nodal = self._entry("stiffness_apply_planned_geom_nodal")

    def _apply(self, x, cell_constants, y, G, dofmap, dphi_t):
        ncell, nd = self._check(dofmap, (("cell_constants", cell_constants),), (("x", x), ("y", y)))
        if self._geom is None:
            self._check_G(G, ncell, nd)
        else:
            xd, xg, pt, wt = self._geom
            # a cell sub-range hands its rows of x_dofs in the G position (int32 [ncell, 8]: cannot be
            # mistaken for a geometric-factor array); otherwise G is ignored (None)
            if isinstance(G, torch.Tensor) and G.dtype == torch.int32:
                xd = G
            self._check_x_dofs(xd, ncell)
            if self.nodal is not None and (self.nodal.numel() != x.numel() or self.nodal.device != x.device):
                raise ValueError(f"the operator's nodal coefficient has {self.nodal.numel()} entries on {self.nodal.device}, "
                                 f"x has {x.numel()} on {x.device}: one value per dof of x")
        if ncell == 0:
            return
        head = (x.data_ptr(), cell_constants.data_ptr(), y.data_ptr())
        tail = (dphi_t.data_ptr(), self.P, int(ncell), _lib.stream_ptr())
        if self.nodal is not None:
            ws, _ = _PLANS.get(dofmap, strips=True)
            _lib.check(self._fn_nodal(x.data_ptr(), cell_constants.data_ptr(), self.nodal.data_ptr(), y.data_ptr(), xg.data_ptr(),
                                      xd.data_ptr(), pt.data_ptr(), wt.data_ptr(), ws.data_ptr(), *tail),
                       "fus_stiffness_apply_planned_geom_nodal")
        elif self._geom is not None:
            ws, _ = _PLANS.get(dofmap, strips=True)
            _lib.check(self._fn_geom(*head, xg.data_ptr(), xd.data_ptr(), pt.data_ptr(), wt.data_ptr(), ws.data_ptr(), *tail),
                       "fus_stiffness_apply_planned_geom")
        elif self._wratio is not None:
            ws, _ = _PLANS.get(dofmap, strips=True)
            _lib.check(self._fn_affine(*head, G.data_ptr(), self._wratio.data_ptr(), ws.data_ptr(), *tail),
                       "fus_stiffness_apply_planned_affine")
        elif _USE_PLAN:
            ws, _ = _PLANS.get(dofmap)
            _lib.check(self._fn_planned(*head, G.data_ptr(), ws.data_ptr(), *tail), "fus_stiffness_apply_planned")
        else:
            _lib.check(self._fn(*head, G.data_ptr(), dofmap.data_ptr(), *tail), "fus_stiffness_apply")

    def prepare(self, dofmap):
        """Set-up, not an apply: build (and cache) the batch plan for ``dofmap`` now instead of
        lazily inside the first apply."""
        _req(dofmap, torch.int32, "dofmap")
        if _USE_PLAN and dofmap.shape[0] > 0:
            _PLANS.get(dofmap, strips=self._geom is not None or self._wratio is not None)

    # numba-cpu flavour: op(x, cell_constants, y, G, dofmap)
    def __call__(self, x, cell_constants, y, G, dofmap):
        if self._dphi is None:
            raise TypeError("this operator was built cuda-style (no dphi); launch it as op[grid, block](..., dphi)")
        self._apply(x, cell_constants, y, G, dofmap, self._dphi)

    # cuda flavour: op[grid, block](x, consts, y, G, dofmap, dphi)
    def launch(self, x, entity_constants, y, G_entity, entity_dofmap, dphi):
        if dphi is not self._dphi_src:  # convert/cache the table once per distinct object
            self._dphi_cuda = self._table(dphi)
            self._dphi_src = dphi
        self._apply(x, entity_constants, y, G_entity, entity_dofmap, self._dphi_cuda)


def stiffness_operator(P, *args, affine_weights=None, geometry=None, nodal=None):
    """``stiffness_operator(P, dphi, float_type)`` (numba-cpu/operators.py:71) or
    ``stiffness_operator(P, float_type)`` (cuda/operators.py:73).

    ``affine_weights`` (keyword, no reference counterpart): opt into the affine-cell fast path by
    passing the tensor quadrature weights ``[n^3]``; the operator then reads only ``G[c, 0, :]`` of
    each cell.  Only valid when every cell is affine (``is_affine_geometry`` checks).

    ``geometry`` (keyword, no reference counterpart): ``(x_dofs, x_g, pts, wts)`` -- the reference's
    mesh pair of numba-cpu/precompute.py:115 plus the 1-D GLL points / weights; the operator then
    forms G in the kernel from the 8 vertices of each (trilinear) cell and ignores its ``G``
    argument.  ``x_dofs`` rows must be in the dofmap's cell order.

    ``nodal`` (keyword, needs ``geometry``; no reference counterpart): a coefficient ``kappa`` with one value per dof of ``x``
    (owned and ghost dofs, the numbering of ``x``).  The operator becomes ``y += K(cell_constants * kappa) x`` with kappa taken at
    the quadrature points, which the GLL rule collocates with the dofs (csrc/stiffness_geom_nodal.hpp); ``cell_constants`` stays
    a factor per cell.  The operator holds kappa as a device tensor of its type (``op.nodal``) and checks its length against
    ``x`` at every apply.  Without ``geometry`` this raises: the general-G kernels compute the same operator from
    ``nodal_medium.scale_G(G, kappa, dofmap)``."""
    if len(args) == 2:
        dphi, float_type = args
        return _StiffnessOperator(P, float_type, dphi, affine_weights, geometry, nodal)
    if len(args) == 1:
        return _StiffnessOperator(P, args[0], None, affine_weights, geometry, nodal)
    raise TypeError("stiffness_operator(P, dphi, float_type) or stiffness_operator(P, float_type)")


class _GradientOperator(_CellOperator):
    """Returned by ``gradient_operator``: ``op(x, cell_constants, y3, dofmap)`` adds the weak gradient C(c) x
    (csrc/gradient_geom.hpp) to the three rows of ``y3``."""

    def __init__(self, P, dphi, float_type, geometry):
        if geometry is None or len(geometry) != 4:
            raise ValueError("gradient_operator needs geometry=(x_dofs, x_g, pts, wts): the gradient is formed from the cell vertices")
        if dphi is None:
            raise ValueError("gradient_operator needs the 1-D derivative table dphi")
        super().__init__(P, float_type, dphi)
        self._geom = (self._check_x_dofs(_to_device(geometry[0], torch.int32), None),) + self._geometry(*geometry[1:])
        self._fn = self._entry("gradient_apply_planned_geom")

    def __call__(self, x, cell_constants, y3, dofmap):
        rows = isinstance(y3, torch.Tensor) and y3.dim() == 2 and y3.shape[0] == 3 and y3.stride(1) == 1
        # rows may be further apart than ndofs (a view): the kernel takes the row stride
        ncell, _ = self._check(dofmap, (("cell_constants", cell_constants),), (("x", x), ("y3", y3[0] if rows else y3)))
        if not rows:
            raise ValueError("y3 must be [3, ndofs] with contiguous rows")
        ystride = y3.stride(0) if y3.shape[1] > 0 else 0
        if x.dim() != 1 or y3.shape[1] != x.numel() or ystride < y3.shape[1]:
            raise ValueError("x must be [ndofs] and y3 [3, ndofs] over the same dofs")
        xd, xg, pt, wt = self._geom
        self._check_x_dofs(xd, ncell)
        if ncell == 0:
            return
        ws, _ = _PLANS.get(dofmap, strips=True)
        _lib.check(
            self._fn(x.data_ptr(), cell_constants.data_ptr(), y3.data_ptr(), int(ystride), xg.data_ptr(), xd.data_ptr(), pt.data_ptr(),
                     wt.data_ptr(), ws.data_ptr(), self._dphi.data_ptr(), self.P, int(ncell), _lib.stream_ptr()),
            "fus_gradient_apply_planned_geom",
        )

    def prepare(self, dofmap):
        """Set-up, not an apply: build (and cache) the batch plan for ``dofmap`` now."""
        _req(dofmap, torch.int32, "dofmap")
        if dofmap.shape[0] > 0:
            _PLANS.get(dofmap, strips=True)


def gradient_operator(P, dphi, float_type, geometry=None):
    """``gradient_operator(P, dphi, float_type, geometry=(x_dofs, x_g, pts, wts))`` -> ``op(x, cell_constants, y3, dofmap)``
    (no reference counterpart).  ``y3[d] += C_d(c) x``, the weak gradient

        y_d[i] += sum_cells c_cell sum_{q: dof(cell, q) = i} w_q |det J_q| (dx / dx_d)(q)

    with the geometry formed in the kernel from the 8 vertices of each (trilinear) cell, in the conventions of
    ``stiffness_operator(..., geometry=)``; ``y3`` is a ``[3, ndofs]`` tensor with contiguous rows (a view whose row stride
    exceeds ``ndofs`` is accepted).  ``y3 / (M(1) 1)`` is the lumped-mass projection of ``c grad x`` (``intensity.recovered_gradient``)."""
    return _GradientOperator(P, dphi, float_type, geometry)


class _WesterveltCellOperator(_CellOperator):
    """Fused Westervelt cell pass (csrc/westervelt.hpp): ``b += K(c3) u + K(c4) v + M(c5) v^2`` and
    ``m += M(c2) u`` in one sweep over the cells -- the four cell launches of
    cuda/demo_nonlinear_bowl.py:612-632 (+ square :603).  No reference counterpart as a single call.
    The body of both forms; ``geometry``: the cell geometry a call hands over, ``(G, detJ)`` here."""

    _entry_name, _strips = "westervelt_cell_apply_planned", False

    def __init__(self, P, dphi, float_type):
        super().__init__(P, float_type, dphi)
        self._fn = self._entry(self._entry_name)

    def _geometry_args(self, geometry, ncell, nd, full):
        G, detJ = geometry
        self._check_G(G, ncell, nd)
        if full:
            _req(detJ, self.dtype, "detJ")
            if detJ.numel() != ncell * nd:
                raise ValueError(f"detJ must be [ncell, {nd}]")
        return G.data_ptr(), detJ.data_ptr() if full else None

    def _apply(self, u, v, c2, c3, c4, c5, b, m, geometry, dofmap):
        """``c2``, ``c5``, ``m`` None: the stiffness part alone."""
        full = c2 is not None
        if full:
            ncell, nd = self._check(dofmap, (("c2", c2), ("c3", c3), ("c4", c4), ("c5", c5)), (("u", u), ("v", v), ("b", b), ("m", m)))
        else:
            ncell, nd = self._check(dofmap, (("c3", c3), ("c4", c4)), (("u", u), ("v", v), ("b", b)))
        geometry = self._geometry_args(geometry, ncell, nd, full)
        if ncell == 0:
            return
        ws, _ = _PLANS.get(dofmap, strips=self._strips)
        _lib.check(
            self._fn(u.data_ptr(), v.data_ptr(), c2.data_ptr() if full else None, c3.data_ptr(), c4.data_ptr(),
                     c5.data_ptr() if full else None, b.data_ptr(), m.data_ptr() if full else None, *geometry, ws.data_ptr(),
                     self._dphi.data_ptr(), self.P, int(ncell), _lib.stream_ptr()),
            "fus_" + self._entry_name if full else "fus_westervelt_cell_apply_planned (stiffness part)",
        )

    def __call__(self, u, v, c2, c3, c4, c5, b, m, G, detJ, dofmap):
        self._apply(u, v, c2, c3, c4, c5, b, m, (G, detJ), dofmap)

    def stiffness_only(self, u, v, c3, c4, b, G, dofmap):
        """``b += K(c3) u + K(c4) v`` in one pass over the cells (G read once, u and v gathered once): the
        stiffness part of the Westervelt stage; the mass terms are applied pointwise by the driver from
        precomputed diagonals (``fus_rk4_stage_nl2_*``)."""
        self._apply(u, v, None, c3, c4, None, b, None, (G, None), dofmap)


class _WesterveltCellGeomOperator(_WesterveltCellOperator):
    """The fused Westervelt cell pass with G and detJ formed in the kernel from the cell vertices
    (csrc/westervelt_geom.hpp): ``op(u, v, c2, c3, c4, c5, b, m, x_dofs, dofmap)``.  ``x_dofs`` (int32
    [ncell, 8], dofmap cell order) is a call argument so that cell sub-ranges can be passed as views;
    ``x_g``, ``pts``, ``wts`` are fixed at construction."""

    _entry_name, _strips = "westervelt_cell_apply_planned_geom", True

    def __init__(self, P, dphi, float_type, x_g, pts, wts):
        super().__init__(P, dphi, float_type)
        self.x_g, self.pts, self.wts = self._geometry(x_g, pts, wts)

    def _geometry_args(self, x_dofs, ncell, nd, full):
        self._check_x_dofs(x_dofs, ncell)
        return self.x_g.data_ptr(), x_dofs.data_ptr(), self.pts.data_ptr(), self.wts.data_ptr()

    def __call__(self, u, v, c2, c3, c4, c5, b, m, x_dofs, dofmap):
        self._apply(u, v, c2, c3, c4, c5, b, m, x_dofs, dofmap)

    def stiffness_only(self, u, v, c3, c4, b, x_dofs, dofmap):
        """As ``_WesterveltCellOperator.stiffness_only`` with G formed in the kernel from the cell vertices."""
        self._apply(u, v, None, c3, c4, None, b, None, x_dofs, dofmap)


class _WesterveltCellNodalOperator(_WesterveltCellGeomOperator):
    """The stiffness part of the Westervelt cell pass with NODAL coefficients (csrc/westervelt_geom_nodal.hpp):
    ``b += sum_q B_q^T G_q (c3 kappa3 grad u + c4 kappa4 grad v)``, G formed in the kernel.  ``kappa3`` / ``kappa4`` (one value per
    dof of ``u``, owned and ghost) are held by the operator as device tensors of its type (``op.nodal``), so that
    ``stiffness_only`` keeps the call shape of the per-cell operator and a cell sub-range of a halo schedule needs nothing new.
    The kernel has no mass part: the full form raises."""

    _entry_name = "westervelt_stiffness_apply_planned_geom_nodal"

    def __init__(self, P, dphi, float_type, x_g, pts, wts, nodal):
        super().__init__(P, dphi, float_type, x_g, pts, wts)
        if len(nodal) != 2:
            raise ValueError("westervelt_cell_operator(nodal=(kappa3, kappa4)): two coefficient vectors")
        self.nodal = tuple(_to_device(k, self.dtype).reshape(-1) for k in nodal)
        if self.nodal[0].numel() != self.nodal[1].numel():
            raise ValueError("westervelt_cell_operator(nodal=(kappa3, kappa4)): the two vectors differ in length")

    def __call__(self, u, v, c2, c3, c4, c5, b, m, x_dofs, dofmap):
        raise ValueError("the nodal Westervelt cell operator has no mass part (c2 / c5 / m): call stiffness_only and take the mass "
                         "terms from diagonals, as the fused stage does")

    def stiffness_only(self, u, v, c3, c4, b, x_dofs, dofmap):
        """``b += K(c3 kappa3) u + K(c4 kappa4) v`` in one pass over the cells."""
        ncell, nd = self._check(dofmap, (("c3", c3), ("c4", c4)), (("u", u), ("v", v), ("b", b)))
        geometry = self._geometry_args(x_dofs, ncell, nd, False)
        k3, k4 = self.nodal
        if k3.numel() != u.numel() or k3.device != u.device or v.numel() != u.numel():
            raise ValueError(f"the operator's nodal coefficients have {k3.numel()} entries on {k3.device}, u has {u.numel()} on "
                             f"{u.device} and v {v.numel()}: one value per dof of u")
        if ncell == 0:
            return
        ws, _ = _PLANS.get(dofmap, strips=self._strips)
        _lib.check(self._fn(u.data_ptr(), v.data_ptr(), c3.data_ptr(), c4.data_ptr(), k3.data_ptr(), k4.data_ptr(), b.data_ptr(),
                            *geometry, ws.data_ptr(), self._dphi.data_ptr(), self.P, int(ncell), _lib.stream_ptr()),
                   "fus_" + self._entry_name)


def westervelt_cell_operator(P, dphi, float_type, geometry=None, nodal=None):
    """``geometry=(x_g, pts, wts)``: the variant that forms G and detJ in the kernel (its call takes
    ``x_dofs`` in place of ``G, detJ``).  ``nodal=(kappa3, kappa4)`` (needs ``geometry``): a coefficient per dof of ``u`` on
    each input, inside the contraction (``_WesterveltCellNodalOperator``; ``stiffness_only`` alone)."""
    if nodal is not None:
        if geometry is None:  # (before anything is put on a device)
            raise ValueError("westervelt_cell_operator(nodal=...) needs geometry=(x_g, pts, wts): the nodal kernel forms G from the "
                             "cell vertices")
        return _WesterveltCellNodalOperator(P, dphi, float_type, *geometry, nodal)
    if geometry is not None:
        return _WesterveltCellGeomOperator(P, dphi, float_type, *geometry)
    return _WesterveltCellOperator(P, dphi, float_type)


def locality_cell_order(dofmap):
    """Set-up helper: permutation of the cells (int64 tensor on the dofmap's device) that puts cells
    with nearby dofs next to each other -- cells sorted by their smallest dof.  The planned kernels
    handle ANY cell order correctly; their speed depends on how many distinct dofs the 256 // n^2
    consecutive cells of a batch touch (tools/exp_numbering.py), which a mesh whose cell order is
    unrelated to its dof numbering loses.  The plan cache applies this order by itself, as an index
    indirection inside the plan (``use_locality_order``); a driver may instead apply it once to every
    per-cell array (``dofmap[perm]``, ``G[perm]``, ``cell_constants[perm]``, ``detJ[perm]``)."""
    _req(dofmap, torch.int32, "dofmap")
    return torch.argsort(dofmap.min(dim=1).values, stable=True)


def is_affine_geometry(G, weights, rtol=1e-12):
    """True if ``G[c, q, :] == G[c, 0, :] * w_q / w_0`` for every cell (set-up check for the
    affine fast path; one pass over G with torch, not part of the apply)."""
    w = torch.as_tensor(np.asarray(weights, dtype=np.float64).reshape(-1), device=G.device).to(G.dtype)
    Gv = G.reshape(G.shape[0], -1, 6)
    ref = Gv[:, :1, :] * (w / w[0]).reshape(1, -1, 1)
    scale = Gv.abs().amax()
    return bool(((Gv - ref).abs().amax() <= rtol * scale).item())


# -------------------------------------------------------------------- vector ops
def _vec(name, *tensors):
    dt = tensors[0].dtype if isinstance(tensors[0], torch.Tensor) else None
    for i, t in enumerate(tensors):
        _req(t, dt, f"arg{i}")
    n = tensors[0].numel()
    return getattr(_lib.load(), f"fus_{name}_{_lib.suffix(dt)}"), n


def _axpy(alpha, x, y, n=None):
    fn, _ = _vec("axpy", x, y)
    n = min(x.numel(), y.numel()) if n is None else int(n)
    if n > x.numel() or n > y.numel():
        raise ValueError("axpy: n exceeds the vector length")
    _lib.check(fn(float(alpha), x.data_ptr(), y.data_ptr(), n, _lib.stream_ptr()), "fus_axpy")


class _Axpy(_Launchable):
    def __call__(self, local_size: int):
        n = int(local_size)

        def kernel(alpha, x, y):
            _axpy(alpha, x, y, n)

        return kernel

    @staticmethod
    def launch(alpha, x, y):
        _axpy(alpha, x, y)


class _Copy(_Launchable):
    @staticmethod
    def launch(a, b):
        fn, n = _vec("copy", a, b)
        if b.numel() < n:
            raise ValueError("copy: output shorter than input")
        _lib.check(fn(a.data_ptr(), b.data_ptr(), n, _lib.stream_ptr()), "fus_copy")

    __call__ = launch


class _Fill(_Launchable):
    @staticmethod
    def launch(alpha, x):
        fn, n = _vec("fill", x)
        _lib.check(fn(float(alpha), x.data_ptr(), n, _lib.stream_ptr()), "fus_fill")

    __call__ = launch


class _PointwiseDivide(_Launchable):
    @staticmethod
    def launch(a, b, c):
        fn, _ = _vec("pointwise_divide", a, b, c)
        n = c.numel()
        if a.numel() < n or b.numel() < n:
            raise ValueError("pointwise_divide: inputs shorter than output")
        _lib.check(fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), n, _lib.stream_ptr()), "fus_pointwise_divide")

    __call__ = launch


class _Square(_Launchable):
    @staticmethod
    def launch(a, b):
        fn, n = _vec("square", a, b)
        if b.numel() < n:
            raise ValueError("square: output shorter than input")
        _lib.check(fn(a.data_ptr(), b.data_ptr(), n, _lib.stream_ptr()), "fus_square")

    __call__ = launch


class _Scale(_Launchable):
    """b = alpha a  (no reference kernel; the drivers here use it for per-stage facet constants)."""

    @staticmethod
    def launch(alpha, a, b):
        fn, n = _vec("scale", a, b)
        if b.numel() < n:
            raise ValueError("scale: output shorter than input")
        _lib.check(fn(float(alpha), a.data_ptr(), b.data_ptr(), n, _lib.stream_ptr()), "fus_scale")

    __call__ = launch


class _MulAdd(_Launchable):
    """y += w * x over the length of y  (``fus_muladd_*``, the kernel of ``DiagonalMassOperator``; no reference kernel: the product
    of a field with an assembled diagonal, which the Westervelt reference sequence with a nodal medium takes in place of a cell mass
    apply)."""

    @staticmethod
    def launch(w, x, y):
        fn, _ = _vec("muladd", w, x, y)
        n = y.numel()
        if w.numel() < n or x.numel() < n:
            raise ValueError("muladd: inputs shorter than output")
        _lib.check(fn(w.data_ptr(), x.data_ptr(), y.data_ptr(), n, _lib.stream_ptr()), "fus_muladd")

    __call__ = launch


axpy = _Axpy()
muladd = _MulAdd()
scale = _Scale()
copy = _Copy()
fill = _Fill()
pointwise_divide = _PointwiseDivide()
square = _Square()
