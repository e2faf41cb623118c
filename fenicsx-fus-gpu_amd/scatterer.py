"""
Ghost-dof halo exchange: ``scatter_reverse`` / ``scatter_forward`` with the
reference's call surface and semantics

    scatter_reverse(comm, owners_data, ghosts_data, N, float_type) -> scatter(buffer)
    scatter_forward(comm, owners_data, ghosts_data, N, float_type) -> scatter(buffer)
        cuda/scatterer.py:104-188, 191-277   (owners_data/ghosts_data: 3-element lists)
        numba-cpu/scatterer.py:78-141, 144-207 (4-element flat lists with offsets)

  reverse: my ghost values -> their owners, ADDED there          (ghost partial sums)
  forward: my owned values -> the ranks that ghost them, COPIED  (ghost refresh)
both in place on ``buffer`` (length nlocal + nghost, ghosts at ``[N:]``).

MI355X-first differences from the reference:
  * one fused pack and one fused unpack launch for ALL neighbours (index lists
    concatenated) instead of one tiny kernel per neighbour;
  * transport = one neighbour all-to-all-v as grouped RCCL send/recv over xGMI
    instead of per-neighbour MPI Isend/Irecv on device pointers; no
    host-blocking device synchronisation anywhere: ordering is by stream and
    events (pack -> exchange -> unpack), so the host runs ahead;
  * split-phase ``begin()`` / ``end()`` so interior-cell operator application
    overlaps the exchange (``HaloApply``, halo_apply.py).

``comm`` selects the transport (comm.py):
  * an ``mpi4py.MPI.Comm`` -- what the reference's drivers pass (cuda/demo_linear_box.py:41, 206-207) -- is accepted as it
    is: it becomes the bootstrap of a ``NativeComm`` (``as_comm``; ``mpi_bootstrap.py``), no ``torch.distributed`` needed;
  * ``NativeComm`` (default of the drivers): the exchange lives in libfusgpu.so
    (csrc/halo_comm.hpp, C ABI ``fus_halo_*``): pack, ``ncclGroupStart ...
    ncclSend/ncclRecv ... ncclGroupEnd`` and unpack are issued from C++ on a
    library-owned high-priority stream; torch.distributed only broadcasts the
    RCCL unique id at start-up;
  * ``TorchComm``: ``torch.distributed.all_to_all_single`` (backend "nccl" == RCCL,
    or "gloo" for CPU tests) with the pack / unpack kernels launched from Python;
    ``kernels`` then selects their implementation: the HIP kernels of libfusgpu.so
    by default (GPU tensors; no CPU fallback) -- tests inject their own for
    gloo-on-CPU runs.
"""


from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .comm import NativeComm, TorchComm, as_comm, bootstrap_of, comm_size, default_comm, gather_arrays, gather_floats, vote  # noqa: F401
from .halo_apply import HaloApply  # noqa: F401
from .utils import to_flat


class _NativeScatter:
    """scatter_forward / scatter_reverse closure over ``fus_halo_*`` (the exchange is issued from C++)."""

    def __init__(self, comm: NativeComm, owners_data, ghosts_data, N, float_type, reverse: bool, halo=None):
        self.comm, self.N, self.reverse = comm, int(N), reverse
        self.dtype = _lib.torch_dtype(float_type)
        lib = _lib.load()
        self._lib = lib
        if halo is not None:  # share the plan + buffers of another closure (same vector never in flight twice)
            self._owner, self.handle = halo, halo.handle
        else:
            o_idx, o_size, _, o_ranks = to_flat(owners_data)
            g_idx, g_size, _, g_ranks = to_flat(ghosts_data)
            self.handle = C.c_void_p()
            self._owner = None

            def arr(a, dt):
                a = np.ascontiguousarray(a, dtype=dt)
                return a, a.ctypes.data_as(C.c_void_p)

            keep = [arr(o_ranks, np.int32), arr(o_size, np.int64), arr(o_idx, np.int64),
                    arr(g_ranks, np.int32), arr(g_size, np.int64), arr(g_idx, np.int64)]
            rc = lib.fus_halo_create(comm.handle, 8 if self.dtype == torch.float64 else 4, self.N, int(len(o_idx)),
                                     len(o_ranks), keep[0][1], keep[1][1], keep[2][1],
                                     len(g_ranks), keep[3][1], keep[4][1], keep[5][1], C.byref(self.handle))
            # PEER, one process per rank: building a closure continues with a collective (the all-gather of the arena
            # handles).  A rank whose object could not be created (out of memory, a bad plan) must not leave the others
            # inside that all-gather: agree on the outcome first, so that the failure is raised on every rank here.
            boot = bootstrap_of(comm)
            if comm.transport == "peer" and not comm.in_process and boot is not None and comm.size > 1:
                vote(boot, rc == 0, "fus_halo_create failed on another rank: no halo object is built on any rank", undo=self.close, own_error=True)
            _lib.check(rc, "fus_halo_create", comm.handle)
            self._index = comm._nhalos
            comm._nhalos += 1
        self.nghost = None
        self.direct = bool(lib.fus_halo_is_direct(self.handle) == 1)
        self.active = True
        sfx = "reverse" if reverse else "forward"
        self._begin, self._end = getattr(lib, f"fus_halo_{sfx}_begin"), getattr(lib, f"fus_halo_{sfx}_end")
        self._whole = getattr(lib, f"fus_halo_{sfx}")
        # PEER transport: map the neighbours' arenas (collective all-gather of the handles; in-process worlds connect
        # at the first exchange, when all ranks exist)
        self._connected = True
        if halo is None and comm.transport == "peer":
            self._connected = comm._peer_connect(self.handle, self._index)

    def _ensure_connected(self):
        owner = self._owner if self._owner is not None else self
        if not owner._connected:
            owner._connected = self.comm._peer_connect(owner.handle, owner._index, lazy_ok=False)

    def status(self):
        """PEER transport: ``{"timeouts": device-side waits that gave up (0 = healthy), ...}`` (synchronises)."""
        if self.comm.transport != "peer":
            return {"failures": 0, "timeouts": 0, "poisoned": 0, "dead": False}
        out = (C.c_int64 * 8)()
        _lib.check(self._lib.fus_halo_ipc_status(self.handle, out), "fus_halo_ipc_status", self.comm.handle)
        return {"failures": int(out[0]), "timeouts": int(out[4]), "poisoned": int(out[5]), "dead": bool(out[6]),
                "forward_posted": int(out[1]), "reverse_posted": int(out[2]),
                "arena_memory": ("fine-grained", "uncached", "ordinary")[int(out[3])],
                "fenced": bool(out[7])}  # FUS_IPC_FENCED=1 at creation: system-scope release / acquire around the flags

    def begin(self, buffer):
        _lib.require_device_tensor(buffer, self.dtype, "buffer")
        self._ensure_connected()
        _lib.check(self._begin(self.handle, buffer.data_ptr(), _lib.stream_ptr()), "fus_halo_begin", self.comm.handle)
        return None

    def end(self, buffer, work=None):
        _lib.check(self._end(self.handle, buffer.data_ptr(), _lib.stream_ptr()), "fus_halo_end", self.comm.handle)

    def __call__(self, buffer):
        """``scatter(buffer)`` of the reference's closures: the whole exchange, in stream order on the caller's stream
        (``fus_halo_forward`` / ``fus_halo_reverse``: the PEER transport then runs its two kernels on that stream itself, no
        event edge to the communicator's stream and back)."""
        _lib.require_device_tensor(buffer, self.dtype, "buffer")
        self._ensure_connected()
        _lib.check(self._whole(self.handle, buffer.data_ptr(), _lib.stream_ptr()), "fus_halo_exchange", self.comm.handle)

    def close(self):
        # a halo must be destroyed before its communicator; if the communicator is already gone
        # (interpreter shutdown order) the handle is dropped without touching it
        if self._owner is None and self.handle:
            if getattr(self.comm, "handle", None):
                self._lib.fus_halo_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipHaloKernels:
    """pack/unpack through the C ABI (csrc/halo.hpp)."""

    def __init__(self, dtype: torch.dtype):
        lib = _lib.load()
        suf = _lib.suffix(dtype)
        self.dtype = dtype
        self._pack_fwd = getattr(lib, f"fus_pack_fwd_{suf}")
        self._unpack_fwd = getattr(lib, f"fus_unpack_fwd_{suf}")
        self._pack_rev = getattr(lib, f"fus_pack_rev_{suf}")
        self._unpack_rev = getattr(lib, f"fus_unpack_rev_{suf}")

    def index_tensor(self, idx_np):
        dev = torch.device("cuda", torch.cuda.current_device())
        return torch.from_numpy(np.ascontiguousarray(idx_np, dtype=np.int64)).to(dev)

    def buffer(self, n):
        return torch.empty(int(n), dtype=self.dtype, device=torch.device("cuda", torch.cuda.current_device()))

    def _chk(self, t, name):
        _lib.require_device_tensor(t, self.dtype, name)

    def pack_fwd(self, in_, out, index):
        self._chk(in_, "buffer")
        _lib.check(self._pack_fwd(in_.data_ptr(), out.data_ptr(), index.data_ptr(), index.numel(), _lib.stream_ptr()), "fus_pack_fwd")

    def unpack_fwd(self, in_, out, index, N):
        self._chk(out, "buffer")
        _lib.check(self._unpack_fwd(in_.data_ptr(), out.data_ptr(), index.data_ptr(), index.numel(), int(N), _lib.stream_ptr()), "fus_unpack_fwd")

    def pack_rev(self, in_, out, index, N):
        self._chk(in_, "buffer")
        _lib.check(self._pack_rev(in_.data_ptr(), out.data_ptr(), index.data_ptr(), index.numel(), int(N), _lib.stream_ptr()), "fus_pack_rev")

    def unpack_rev(self, in_, out, index):
        self._chk(out, "buffer")
        _lib.check(self._unpack_rev(in_.data_ptr(), out.data_ptr(), index.data_ptr(), index.numel(), _lib.stream_ptr()), "fus_unpack_rev")


class _Scatter:
    """Callable returned by scatter_forward / scatter_reverse."""

    def __init__(self, comm, owners_data, ghosts_data, N, float_type, reverse: bool, kernels=None):
        self.comm = comm
        self.N = int(N)
        self.reverse = reverse
        tdt = _lib.torch_dtype(float_type)
        self.k = kernels if kernels is not None else HipHaloKernels(tdt)
        o_idx, o_size, _, o_ranks = to_flat(owners_data)
        g_idx, g_size, _, g_ranks = to_flat(ghosts_data)
        size = comm.size
        o_counts = [0] * size
        g_counts = [0] * size
        for r, c in zip(o_ranks, o_size):
            o_counts[int(r)] = int(c)
        for r, c in zip(g_ranks, g_size):
            g_counts[int(r)] = int(c)
        # the flat index lists are grouped by ascending neighbour rank, which is the segment
        # order all_to_all_single uses
        assert list(o_ranks) == sorted(o_ranks) and list(g_ranks) == sorted(g_ranks)
        self.o_idx = self.k.index_tensor(o_idx)
        self.g_idx = self.k.index_tensor(g_idx)
        if reverse:  # ghosts -> owners
            self.send_counts, self.recv_counts = o_counts, g_counts
        else:  # owners -> ghosts
            self.send_counts, self.recv_counts = g_counts, o_counts
        # send/recv buffers are owned by the closure and allocated once (cuda/scatterer.py:133-138)
        self.send = self.k.buffer(sum(self.send_counts))
        self.recv = self.k.buffer(sum(self.recv_counts))
        # ghosts numbered owner by owner (BoxMesh does; a dolfinx mesh may not): the ghost block of
        # the vector IS the message buffer of the owners' side -- receive into it (forward) / send
        # from it (reverse) directly, no unpack_fwd / pack_rev launch
        self.nghost = int(len(o_idx))
        self.direct = self.nghost > 0 and bool(np.array_equal(np.asarray(o_idx), np.arange(self.nghost)))
        self.active = (sum(self.send_counts) + sum(self.recv_counts)) > 0 or comm.size > 1

    def begin(self, buffer):
        """Pack and post the exchange; returns a handle for ``end``."""
        send, recv = self.send, self.recv
        if self.reverse:
            if self.direct:
                send = buffer[self.N : self.N + self.nghost]
            else:
                self.k.pack_rev(buffer, self.send, self.o_idx, self.N)
        else:
            self.k.pack_fwd(buffer, self.send, self.g_idx)
            if self.direct:
                recv = buffer[self.N : self.N + self.nghost]
        if self.comm.size == 1:
            return None
        return self.comm.alltoallv(send, self.send_counts, recv, self.recv_counts, async_op=True)

    def end(self, buffer, work):
        """Complete the exchange (stream-ordered for RCCL) and unpack."""
        if work is not None:
            work.wait()
        if self.reverse:
            self.k.unpack_rev(self.recv, buffer, self.g_idx)
        elif not self.direct:
            self.k.unpack_fwd(self.recv, buffer, self.o_idx, self.N)

    def __call__(self, buffer):
        self.end(buffer, self.begin(buffer))


def begin_all(pairs, arm_join=None):
    """Post the exchanges of several ``(scatter closure, vector)`` pairs; returns ``[(closure, vector, handle)]``
    for ``closure.end(vector, handle)``.  Native closures of one communicator and one direction go out as ONE
    RCCL group (``fus_halo_*_begin_group``): the RK4 stage's two forward scatters cost one launch, not two.

    ``arm_join`` (a ``NativeComm``): these exchanges are the LAST work of an apply on the communicator's stream; the receive
    kernel of the last one publishes the join flag (``fus_comm_arm_join``).  The library hands the join to the last halo of
    ONE begin call, so it is armed right before the call that posts the last exchange -- the group, or, when the pairs go out
    one by one (more than 8, mixed closures), the last ``begin`` (armed before the first of several calls, the
    first receive kernel would publish the flag while the later exchanges are still queued)."""
    pairs = list(pairs)
    native = [sc for sc, _ in pairs if isinstance(sc, _NativeScatter)]
    if len(pairs) > 1 and len(native) == len(pairs) and len({id(sc.comm) for sc in native}) == 1 \
            and len({sc.reverse for sc in native}) == 1 and len(pairs) <= 8:
        for sc, vec in pairs:
            _lib.require_device_tensor(vec, sc.dtype, "buffer")
            sc._ensure_connected()
        halos = (C.c_void_p * len(pairs))(*[sc.handle for sc, _ in pairs])
        bufs = (C.c_void_p * len(pairs))(*[vec.data_ptr() for _, vec in pairs])
        fn = getattr(_lib.load(), "fus_halo_reverse_begin_group" if native[0].reverse else "fus_halo_forward_begin_group")
        if arm_join is not None and native[0].comm is arm_join:
            arm_join.arm_join()
        _lib.check(fn(halos, bufs, len(pairs), _lib.stream_ptr()), "fus_halo_begin_group", native[0].comm.handle)
        return [(sc, vec, None) for sc, vec in pairs]
    out = []
    for i, (sc, vec) in enumerate(pairs):
        if arm_join is not None and i == len(pairs) - 1 and isinstance(sc, _NativeScatter) and sc.comm is arm_join:
            sc._ensure_connected()  # nothing that can fail between arming and the begin that takes the join
            arm_join.arm_join()
        out.append((sc, vec, sc.begin(vec)))
    return out


def _make_scatter(comm, owners_data, ghosts_data, N, float_type, kernels, reverse):
    comm = as_comm(comm)
    if isinstance(comm, NativeComm):
        return _NativeScatter(comm, owners_data, ghosts_data, N, float_type, reverse)
    return _Scatter(comm, owners_data, ghosts_data, N, float_type, reverse, kernels)


def scatter_reverse(comm, owners_data, ghosts_data, N, float_type, kernels=None):
    """cuda/scatterer.py:104-188 / numba-cpu/scatterer.py:78-141.  ``comm``: see ``as_comm`` (an ``MPI.Comm`` is accepted)."""
    return _make_scatter(comm, owners_data, ghosts_data, N, float_type, kernels, True)


def scatter_forward(comm, owners_data, ghosts_data, N, float_type, kernels=None):
    """cuda/scatterer.py:191-277 / numba-cpu/scatterer.py:144-207.  ``comm``: see ``as_comm`` (an ``MPI.Comm`` is accepted)."""
    return _make_scatter(comm, owners_data, ghosts_data, N, float_type, kernels, False)
