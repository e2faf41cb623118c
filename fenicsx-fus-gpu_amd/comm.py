"""
Communicators of the halo exchange and their bootstrap plumbing: ``TorchComm``, ``NativeComm``, what a driver's ``comm``
becomes (``default_comm``, ``as_comm``) and the set-up gathers.  ``scatterer.py`` says which transport each one selects, has
the scatter closures that run on them and re-exports every name defined here.
"""

from __future__ import annotations

import ctypes as C
import io
import os
import struct

import numpy as np
import torch
import torch.distributed as dist

from . import _lib


class TorchComm:
    """Thin communicator over a ``torch.distributed`` process group
    (backend "nccl" == RCCL on ROCm; "gloo" for CPU tests)."""

    def __init__(self, group=None):
        self.group = group
        self.rank = dist.get_rank(group)
        self.size = dist.get_world_size(group)
        self.backend = dist.get_backend(group)

    def _device(self):
        """Where the collectives' tensors live: the current GPU for RCCL, the host for gloo."""
        return torch.device("cuda", torch.cuda.current_device()) if self.backend == "nccl" else torch.device("cpu")

    def alltoallv(self, send, send_counts, recv, recv_counts, async_op=False):
        """Neighbour all-to-all-v: ``send`` / ``recv`` are flat tensors whose
        consecutive segments (``*_counts[r]`` elements, zero for non-neighbours)
        go to / come from rank r."""
        return dist.all_to_all_single(
            recv, send, output_split_sizes=recv_counts, input_split_sizes=send_counts, group=self.group, async_op=async_op
        )

    def alltoallv_int64(self, send_np, send_counts, recv_counts):
        """Set-up path (index exchange of compute_scatterer_data)."""
        dev = self._device()
        send = torch.from_numpy(np.ascontiguousarray(send_np, dtype=np.int64)).to(dev)
        recv = torch.empty(int(np.sum(recv_counts)), dtype=torch.int64, device=dev)
        self.alltoallv(send, [int(c) for c in send_counts], recv, [int(c) for c in recv_counts])
        return recv.cpu().numpy()

    def barrier(self):
        dist.barrier(group=self.group)

    def all_ok(self, ok: bool) -> bool:
        """True iff ``ok`` on EVERY rank (one all-reduce): lets a set-up step fail on all ranks together instead of
        leaving the healthy ones inside the next collective."""
        t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=self._device())
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=self.group)
        return bool(t.item() == 1.0)

    def bcast_bytes(self, payload: bytes, root: int = 0) -> bytes:
        """``payload`` of group rank ``root`` on every rank (same length everywhere: the 128-byte RCCL unique id)."""
        t = torch.frombuffer(bytearray(payload), dtype=torch.uint8).clone().to(self._device())
        dist.broadcast(t, src=dist.get_global_rank(self.group, root) if self.group is not None else root, group=self.group)
        return bytes(t.cpu().numpy().tobytes())

    def allgather_bytes(self, payload: bytes):
        """Every rank's ``payload`` (host bytes of any length), as a list indexed by rank."""
        dev = self._device()
        n = torch.tensor([len(payload)], dtype=torch.int64, device=dev)
        sizes = [torch.zeros_like(n) for _ in range(self.size)]
        dist.all_gather(sizes, n, group=self.group)
        sizes = [int(t.item()) for t in sizes]
        mx = max(max(sizes), 1)
        buf = torch.zeros(mx, dtype=torch.uint8)
        buf[: len(payload)] = torch.frombuffer(bytearray(payload), dtype=torch.uint8) if payload else buf[:0]
        out = [torch.zeros(mx, dtype=torch.uint8, device=dev) for _ in range(self.size)]
        dist.all_gather(out, buf.to(dev), group=self.group)
        return [bytes(t.cpu().numpy()[:sz].tobytes()) for t, sz in zip(out, sizes)]


def vote(boot, ok, message, undo=None, own_error=False):
    """Fail on all ranks or on none: the ranks of ``boot`` (an object with ``all_ok``) agree on ``ok``; unless it holds on every
    rank, ``FusGpuError(message)`` on every rank, after ``undo()`` on those where the step itself went through.  ``own_error``:
    a rank where it did not returns instead, to raise the error of its failed call."""
    if not boot.all_ok(bool(ok)):
        if ok and undo is not None:
            undo()
        if ok or not own_error:
            raise _lib.FusGpuError(message)


class NativeComm:
    """Communicator owned by libfusgpu.so (RCCL over xGMI; csrc/halo_comm.hpp).

    ``NativeComm()``: one rank per process / GPU.  The 128-byte RCCL unique id is created on rank 0
    and broadcast through the default ``torch.distributed`` group (any backend: it is 128 bytes of
    host data), which also carries the one-off integer index exchange of
    ``compute_scatterer_data``; in a 1-rank world no process group is needed.
    ``NativeComm(local=(world_id, nranks, rank))``: all ranks in THIS process (tests on a one-GPU
    box), transport = stream-ordered device copies; every rank's ``begin`` of an exchange must be
    called before any rank's ``end``.

    ``transport="peer"`` (csrc/halo_ipc.hpp): no RCCL.  Each scatter closure owns a receive arena in uncached
    device memory whose HIP IPC handle goes once to its neighbours (all-gathered through ``torch.distributed``, any
    backend); an exchange is a send kernel that stores straight into the neighbours' arenas and a receive kernel that
    waits for a sequence flag -- small kernels that run NEXT TO a chip-filling operator launch, which RCCL's
    264-register kernel does not.  With ``local=...`` the ranks of one process use the same protocol (their arenas
    are plain pointers to each other); the closures connect at their first exchange, when every rank has been built.
    ``hosted=[ranks]`` with ``local=...`` and ``transport="peer"``: THIS process drives only those ranks of the world and
    the other ranks live in other processes of the ``torch.distributed`` group (one process driving several GPUs, or --
    tests -- the 8-rank 2x2x2 partition on 4 processes where the pool allows no more): the processes all-gather the
    arena handles of their ranks once per closure; neighbours of the same process are reached through plain pointers,
    the others through HIP IPC mappings, by the same kernels.  Every process must build its closures in the same order."""

    _peer_local = {}  # (world_id, halo index) -> {rank: blob}: in-process PEER worlds
    _peer_gathered = {}  # (world_id, halo index) -> {rank: blob} of ALL processes (hybrid worlds: gathered once per process)

    def __init__(self, group=None, local=None, transport="rccl", hosted=None, bootstrap=None):
        """``bootstrap``: the object that carries the one-off set-up collectives (rank / size, the votes, the all-gather of
        the arena handles or the broadcast of the RCCL id, the index exchange) instead of the default ``torch.distributed``
        group -- ``mpi_bootstrap.MpiBootstrap(MPI.COMM_WORLD)`` in an ``mpirun`` world (``as_comm`` builds it from a raw
        MPI communicator)."""
        if transport not in ("rccl", "peer"):
            raise ValueError(f"transport must be 'rccl' or 'peer', got {transport!r}")
        lib = _lib.load()
        self._lib = lib
        self.handle = C.c_void_p()
        self.bootstrap = None  # carries the set-up collectives: a TorchComm, an MpiBootstrap (same methods), or nothing
        self.transport = transport
        self._stream = None
        self._world_id = None
        self._nhalos = 0
        self._hosted = None
        if local is not None:
            world_id, self.size, self.rank = (int(v) for v in local)
            self._world_id = world_id
            if hosted is not None:
                if transport != "peer":
                    raise ValueError("hosted= needs transport='peer'")
                self._hosted = sorted(int(r) for r in hosted)
                if self.rank not in self._hosted:
                    raise ValueError(f"rank {self.rank} is not among the hosted ranks {self._hosted}")
                if len(self._hosted) < self.size:
                    if not (dist.is_available() and dist.is_initialized()):
                        raise _lib.FusGpuError("NativeComm(hosted=...): the other ranks' arena handles travel over torch.distributed")
                    self.bootstrap = TorchComm(group)
            if transport == "peer":
                self.backend = "peer-local"
                _lib.check(lib.fus_comm_create_peer(self.size, self.rank, C.byref(self.handle)), "fus_comm_create_peer")
            else:
                self.backend = "local"
                _lib.check(lib.fus_comm_create_local(world_id, self.size, self.rank, C.byref(self.handle)), "fus_comm_create_local")
            return
        if bootstrap is not None:
            self.bootstrap = bootstrap
            self.rank, self.size = int(bootstrap.rank), int(bootstrap.size)
        elif dist.is_available() and dist.is_initialized():
            self.bootstrap = TorchComm(group)
            self.rank, self.size = self.bootstrap.rank, self.bootstrap.size
        else:
            self.rank, self.size = 0, 1
        if transport == "peer":
            self.backend = "peer"
            _lib.check(lib.fus_comm_create_peer(self.size, self.rank, C.byref(self.handle)), "fus_comm_create_peer")
            return
        self.backend = "rccl"
        # Bootstrap that fails on ALL ranks or on none: (1) every rank probes librccl (dlopen + ncclGetUniqueId; only
        # rank 0's id is used) and the ranks agree on the outcome BEFORE anything is broadcast; (2) rank 0's id is
        # broadcast; (3) ncclCommInitRank, then the ranks agree again before any of them proceeds.
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        rc = lib.fus_comm_unique_id(buf)
        err = None if rc == 0 else f"fus_comm_unique_id: {lib.fus_error_string(rc).decode()}: {(lib.fus_comm_last_error(None) or b'?').decode()}"
        if self.size > 1:
            vote(self.bootstrap, err is None, f"RCCL is not usable on every rank (this rank: {err or 'ok'}): no native communicator")
        if err is not None:
            raise _lib.FusGpuError(err)
        raw = bytes(buf.raw)
        if self.size > 1:
            raw = self.bootstrap.bcast_bytes(raw, 0)
        rc = lib.fus_comm_create(raw, self.size, self.rank, C.byref(self.handle))
        err = None if rc == 0 else f"fus_comm_create: {lib.fus_error_string(rc).decode()}: {(lib.fus_comm_last_error(None) or b'?').decode()}"
        if self.size > 1:
            vote(self.bootstrap, err is None, f"ncclCommInitRank did not succeed on every rank (this rank: {err or 'ok'})", undo=self.close)
        if err is not None:
            raise _lib.FusGpuError(err)

    def alltoallv_int64(self, send_np, send_counts, recv_counts):
        """Set-up path (index exchange of compute_scatterer_data): through the bootstrap."""
        if self.bootstrap is None:
            raise _lib.FusGpuError("NativeComm: the index exchange of a multi-rank world needs a bootstrap (torch.distributed or an MPI communicator)")
        return self.bootstrap.alltoallv_int64(send_np, send_counts, recv_counts)

    def barrier(self):
        if self.bootstrap is not None:
            self.bootstrap.barrier()

    @property
    def in_process(self):
        """True for the ranks of a ``local=`` world: driven, with others, from this process."""
        return self._world_id is not None

    def close(self):
        if self.handle:
            if self._lib.fus_comm_destroy(self.handle) == 0:  # refused while halo objects are alive
                self.handle = None
        if self._world_id is not None and self.transport == "peer":
            for key in [k for k in NativeComm._peer_local if k[0] == self._world_id]:
                NativeComm._peer_local[key].pop(self.rank, None)
                if not NativeComm._peer_local[key]:
                    del NativeComm._peer_local[key]
                    NativeComm._peer_gathered.pop(key, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self):
        """The library-owned high-priority stream the exchanges run on, as a torch stream (``fus_comm_stream``)."""
        if self._stream is None:
            ptr = self._lib.fus_comm_stream(self.handle)
            self._stream = torch.cuda.ExternalStream(int(ptr)) if ptr else None
        return self._stream

    def fork(self, lazy=False, attach=False):
        """Order the communicator's stream after the caller's current stream, without an event (``fus_comm_fork_ex``).
        ``lazy`` (PEER transport): no wait kernel -- the first send kernel of the exchange the caller posts NEXT on the
        communicator's stream waits for the fork flag itself.  ``attach``: no signal kernel -- the next PLANNED operator
        launch on the caller's stream publishes the flag when it starts (``fork_flush()`` if none follows)."""
        flags = (_lib.FORK_LAZY if lazy else 0) | (_lib.FORK_ATTACH if attach else 0)
        _lib.check(self._lib.fus_comm_fork_ex(self.handle, _lib.stream_ptr(), flags), "fus_comm_fork", self.handle)

    def fork_flush(self):
        """Publish an attached fork signal that no planned launch has carried (``fus_comm_fork_flush``)."""
        _lib.check(self._lib.fus_comm_fork_flush(self.handle), "fus_comm_fork_flush", self.handle)

    def arm_join(self):
        """PEER transport: the last receive kernel of the exchange posted next publishes the join flag, so that ``join()``
        launches only its wait kernel (``fus_comm_arm_join``).  A no-op for the other transports."""
        _lib.check(self._lib.fus_comm_arm_join(self.handle), "fus_comm_arm_join", self.handle)

    def join(self):
        """Order the caller's current stream after the communicator's stream, without an event (``fus_comm_join``)."""
        _lib.check(self._lib.fus_comm_join(self.handle, _lib.stream_ptr()), "fus_comm_join", self.handle)

    def health(self):
        """Failed device-side waits (time-outs + poisoned flags) of every live halo object of this communicator and of its
        fork / join kernels: 0 = every exchange so far delivered (``fus_comm_health``; synchronises the exchange streams)."""
        n = C.c_int64(0)
        _lib.check(self._lib.fus_comm_health(self.handle, C.byref(n)), "fus_comm_health", self.handle)
        return int(n.value)

    def health_detail(self):
        """``{"timeouts", "poisoned", "sync_timeouts"}``: what ``health()`` adds up."""
        out = (C.c_int64 * 3)()
        _lib.check(self._lib.fus_comm_health_detail(self.handle, out), "fus_comm_health_detail", self.handle)
        return {"timeouts": int(out[0]), "poisoned": int(out[1]), "sync_timeouts": int(out[2])}

    def sync_timeouts(self):
        n = C.c_int64(0)
        _lib.check(self._lib.fus_comm_sync_timeouts(self.handle, C.byref(n)), "fus_comm_sync_timeouts", self.handle)
        return int(n.value)

    # ---- PEER transport: hand a halo object's arena handle to its neighbours
    def _peer_blobs(self, mine, index, lazy_ok):
        """The arena blobs of halo object number ``index`` of all ``size`` ranks, in rank order (``mine``: this rank's), or
        ``None`` if (in-process world) some rank has not built its object yet."""
        if self._world_id is None:
            return self.bootstrap.allgather_bytes(mine) if self.bootstrap is not None else [mine]
        key = (self._world_id, index)
        reg = NativeComm._peer_local.setdefault(key, {})
        if self.rank in reg and reg[self.rank] != mine:  # a new world re-uses the id: drop the old world's handles
            reg.clear()
        reg[self.rank] = mine
        hosted = self._hosted if self._hosted is not None else list(range(self.size))
        if any(r not in reg for r in hosted):
            if lazy_ok:
                return None
            raise _lib.FusGpuError(f"PEER halo {index}: only ranks {sorted(reg)} of {hosted} have built their closure")
        if len(hosted) == self.size:
            return [reg[r] for r in range(self.size)]
        # hybrid world: the rank of this process that completes the set all-gathers the processes' blobs (a
        # collective: every process builds its closures in the same order); the others find them cached
        got = NativeComm._peer_gathered.get(key)
        if got is None or any(got.get(r) != reg[r] for r in hosted):
            payload = b"".join(struct.pack("<q", len(reg[r])) + reg[r] for r in hosted)
            got = {}
            for chunk in self.bootstrap.allgather_bytes(payload):
                off = 0
                while off < len(chunk):
                    (n,) = struct.unpack_from("<q", chunk, off)
                    b = chunk[off + 8: off + 8 + n]
                    got[struct.unpack_from("<Iiii", b)[2]] = b  # IpcBlobHeader: magic, version, rank, ...
                    off += 8 + n
            NativeComm._peer_gathered[key] = got
        missing = [r for r in range(self.size) if r not in got]
        if missing:
            raise _lib.FusGpuError(f"PEER halo {index}: no process hosts rank(s) {missing}")
        return [got[r] for r in range(self.size)]

    def _peer_connect(self, halo_handle, index, lazy_ok=True):
        """Connect halo object number ``index`` of this rank with the other ranks' object number ``index``.
        Returns False if (in-process world) some rank has not built its object yet: retried at the first exchange."""
        lib = self._lib
        n = int(lib.fus_halo_ipc_blob_bytes(halo_handle))
        if n <= 0:
            raise _lib.FusGpuError("fus_halo_ipc_blob_bytes failed")
        buf = C.create_string_buffer(n)
        _lib.check(lib.fus_halo_ipc_export(halo_handle, buf), "fus_halo_ipc_export", self.handle)
        blobs = self._peer_blobs(bytes(buf.raw), index, lazy_ok)
        if blobs is None:
            return False
        keep = [C.create_string_buffer(b, len(b)) for b in blobs]
        arr = (C.c_void_p * len(keep))(*[C.cast(k, C.c_void_p) for k in keep])
        rc = lib.fus_halo_ipc_connect(halo_handle, len(keep), arr)
        if self._world_id is None and self.bootstrap is not None:
            # a rank that cannot map a neighbour's arena must not leave the others waiting for its messages
            detail = (lib.fus_comm_last_error(self.handle) or b"").decode() if rc != 0 else "ok here"
            vote(self.bootstrap, rc == 0, f"PEER halo {index}: mapping the neighbours' arenas did not succeed on every rank ({detail})")
        _lib.check(rc, "fus_halo_ipc_connect", self.handle)
        return True


def default_comm(group=None):
    """The communicator a driver should use at N > 1 (one process per GPU): the PEER transport of libfusgpu.so unless
    ``FUS_HALO=native`` (grouped RCCL send / recv) or ``FUS_HALO=torch`` (``all_to_all_single``).  Bootstrap: the
    ``torch.distributed`` group if one is initialised; otherwise ``MPI.COMM_WORLD`` when mpi4py is importable (a driver
    started with ``mpirun``, as the reference's are: cuda/demo_linear_box.py:41); otherwise a one-rank world.  Creation fails
    on all ranks or on none."""
    kind = os.environ.get("FUS_HALO", "peer")
    if dist.is_available() and dist.is_initialized():
        if kind == "torch":
            return TorchComm(group)
        return NativeComm(group, transport="peer" if kind == "peer" else "rccl")
    from . import mpi_bootstrap

    world = mpi_bootstrap.world_if_available()
    if world is not None:
        return as_comm(world)
    return NativeComm(transport="peer" if kind != "native" else "rccl")


_MPI_COMMS = {}  # id(MPI communicator) -> (the communicator itself, its NativeComm): one library communicator per MPI communicator


def as_comm(comm):
    """The package communicator behind whatever a driver passes as ``comm``:

      * ``NativeComm`` / ``TorchComm`` (or a stand-in with their ``rank`` / ``size`` / ``alltoallv`` members): itself;
      * an ``mpi4py.MPI.Comm`` -- what the reference's drivers pass (cuda/demo_linear_box.py:41, 206-207;
        cuda/scatterer.py:104-110): a ``NativeComm`` bootstrapped over it (``mpi_bootstrap.MpiBootstrap``), transport PEER
        unless ``FUS_HALO=native`` (RCCL); built once per MPI communicator (collectively: every rank must pass it at the same
        point, as every rank of the reference's driver reaches its ``scatter_reverse(comm, ...)`` line);
      * ``None``: ``None``.

    Anything else raises ``TypeError`` naming the accepted kinds."""
    from . import mpi_bootstrap

    if comm is None or isinstance(comm, (NativeComm, TorchComm)):
        return comm
    if mpi_bootstrap.is_mpi_comm(comm):
        hit = _MPI_COMMS.get(id(comm))
        if hit is None or hit[0] is not comm or not hit[1].handle:
            kind = os.environ.get("FUS_HALO", "peer")
            hit = (comm, NativeComm(transport="rccl" if kind == "native" else "peer", bootstrap=mpi_bootstrap.MpiBootstrap(comm)))
            _MPI_COMMS[id(comm)] = hit
        return hit[1]
    if isinstance(getattr(comm, "rank", None), int) and isinstance(getattr(comm, "size", None), int) and \
            (comm.size == 1 or callable(getattr(comm, "alltoallv", None))):
        return comm  # a TorchComm-shaped object (tests, bench.py's staged rehearsal communicator)
    raise TypeError(f"comm: expected a NativeComm, a TorchComm, or an MPI communicator (mpi4py.MPI.Comm: Get_rank / Get_size / allgather / "
                    f"alltoall / bcast), got {type(comm).__name__}")


def bootstrap_of(comm):
    """What carries ``comm``'s set-up collectives: a ``NativeComm``'s bootstrap (``None`` for ranks driven from one process and
    for a one-rank world), a communicator with an ``allgather_bytes`` of its own (``TorchComm``) itself, otherwise ``None``."""
    if hasattr(comm, "handle"):  # a NativeComm
        return comm.bootstrap
    return comm if hasattr(comm, "allgather_bytes") else None


def comm_size(comm):
    """The number of ranks a gather over ``comm`` spans (``None``: one)."""
    return int(getattr(comm, "size", 1))


def gather_arrays(comm, arrays, what, instead):
    """The named numpy ``arrays`` of every rank through the communicator's bootstrap (``allgather_bytes``): one dict per rank, in
    rank order.  Ranks driven from one process have none: ``ValueError`` naming the caller (``what``) and what to use ``instead``."""
    boot = bootstrap_of(comm)
    if boot is None:
        raise ValueError(f"{what}: this communicator has no bootstrap (ranks in one process): use {instead}")
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    out = []
    for blob in boot.allgather_bytes(buf.getvalue()):
        with np.load(io.BytesIO(blob), allow_pickle=False) as z:
            out.append({k: z[k] for k in z.files})
    return out


def gather_floats(comm, values):
    """Every rank's ``values`` (a few host floats) as a float64 array [size, len(values)] in rank order: the solvers' set-up agreements.
    Through a ``NativeComm``'s bootstrap or a ``TorchComm``'s own ``allgather_bytes``; a stand-in with neither (rehearsal over gloo): the
    default ``torch.distributed`` group if initialised.  No communicator, one rank, ranks of one process without a bootstrap: the local row."""
    v = [float(x) for x in values]
    boot = bootstrap_of(comm)
    if boot is None and comm is not None and not hasattr(comm, "handle") and dist.is_available() and dist.is_initialized():
        boot = TorchComm()
    if boot is None or getattr(comm, "size", None) == 1:
        return np.asarray([v], dtype=np.float64)
    return np.asarray([struct.unpack(f"<{len(v)}d", b) for b in boot.allgather_bytes(struct.pack(f"<{len(v)}d", *v))], dtype=np.float64)
