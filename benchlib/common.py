"""What every part of the bench shares: the repo root, the roofline's denominator, stderr logging, the ONE JSON line on
stdout, the watchdog, host-core count, hashes that tie a line to the library / kernel sources it ran."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md)


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


_JSON_FD = None


def protect_stdout():
    """The contract is ONE JSON line on stdout.  Native libraries loaded below write there too (RCCL
    prints a version banner on stdout when a communicator is created with ncclCommInitRank), so file
    descriptor 1 is pointed at stderr for the life of the process and the JSON line is written to a
    private duplicate of the original stdout."""
    global _JSON_FD
    if _JSON_FD is None:
        sys.stdout.flush()
        _JSON_FD = os.dup(1)
        os.dup2(2, 1)


def emit(obj):
    line = (json.dumps(obj) + "\n").encode()
    if _JSON_FD is None:
        sys.stdout.write(line.decode())
        sys.stdout.flush()
    else:
        os.write(_JSON_FD, line)


def start_watchdog(seconds, rank):
    """A rank that is still running after ``seconds`` is taken to be hung (a collective whose peer never
    arrived, a kernel that never drains): say so and leave with a non-zero code, so that the launcher
    stops the other ranks and the caller sees a failure instead of a job that never ends."""
    import threading

    if seconds <= 0:
        return

    def fire():
        log(f"rank {rank}: watchdog: still running after {seconds:.0f} s -- giving up (FUS_BENCH_WATCHDOG_S=0 disables)")
        os._exit(124)

    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()


def host_cores():
    """Cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def lib_sha():
    """Short hash of the libfusgpu.so this run loads (ties a bench line to the profiled binary)."""
    import hashlib

    import fusgpu_loader

    path = fusgpu_loader.submodule("_lib").LIB_PATH
    try:
        with open(path, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:12]
    except OSError:
        return None


def kernel_src_sha(files=("plan.hpp", "stiffness.hpp", "stiffness_plan.hpp")):
    """Hash of what defines a kernel's code (its sources and the compile flags; default: the HEADLINE kernel): a PMC pass
    stays valid for a library that differs from the profiled one only elsewhere (halo transport, ABI glue)."""
    import hashlib

    csrc = os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc")
    h = hashlib.sha256()
    try:
        for n in ("Makefile",) + tuple(files):
            with open(os.path.join(csrc, n), "rb") as f:
                data = f.read()
            if n == "Makefile":  # only the compile flags: the header list changes with every new file
                data = b"\n".join(line for line in data.split(b"\n") if line.startswith((b"CXXFLAGS", b"ARCH", b"           -f")))
            h.update(data)
    except OSError:
        return None
    return h.hexdigest()[:12]


def lib_built_from_tree():
    """True if the loaded libfusgpu.so was built from exactly the sources in this tree (fus_source_hash())."""
    import fusgpu_loader

    try:
        return bool(fusgpu_loader.submodule("_lib").built_from_tree())
    except Exception:
        return None


def _free_port():
    """A free TCP port for the rendezvous, taken from BELOW the kernel's ephemeral range: a port the kernel hands out
    (bind to port 0) is free only until the next outgoing connection takes it, and the ranks that retry connecting to
    it while rank 0 is still starting are such connections (a retry that draws the port itself connects to itself,
    and rank 0 then fails with EADDRINUSE)."""
    import random
    import socket

    try:
        with open("/proc/sys/net/ipv4/ip_local_port_range") as f:
            low = int(f.read().split()[0])
    except (OSError, ValueError, IndexError):
        low = 32768
    hi = max(1025, low)
    lo = max(1024, min(10000, hi - 1000))
    rng = random.Random()  # seeded from the OS: concurrent launchers draw different ports
    for _ in range(200):
        p = rng.randrange(lo, hi)
        with socket.socket() as s:
            try:
                s.bind(("127.0.0.1", p))
            except OSError:
                continue
        return p
    with socket.socket() as s:  # nothing free below the ephemeral range: the kernel's choice
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


DUMP_BUDGET_BYTES = 48 << 20  # --dump-outputs writes at most this much in all (the contract allows 64 MB)


def dump_outputs(directory, arrays, budget=DUMP_BUDGET_BYTES, seed=20240601):
    """``--dump-outputs DIR``: write each array of ``arrays`` (name -> host array) as ``DIR/<name>.npy`` in float32 /
    float64.  Together they stay within ``budget`` bytes: an array that does not fit its share keeps a fixed sample of
    its entries -- the same sorted indices for the same length and seed, so two builds run with the same arguments are
    compared entry for entry.  Returns {name: what was written}."""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v).reshape(-1) for k, v in arrays.items()}
    share = budget // max(1, len(arrays))
    written = {}
    for name, a in arrays.items():
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        keep = share // a.itemsize
        if a.size > keep:
            idx = np.sort(np.random.default_rng(seed).choice(a.size, size=keep, replace=False))
            a = a[idx]
            written[name] = f"{keep} of {arrays[name].size} entries (sorted indices drawn with numpy default_rng({seed}))"
        else:
            written[name] = f"all {a.size} entries"
        np.save(os.path.join(directory, name + ".npy"), a)
    log(f"outputs written to {directory}: {written}")
    return written


def rehearsal():
    """FUS_BENCH_REHEARSAL=1: the N-rank code path of THIS script with real HIP kernels and real processes
    where only one GPU exists -- every rank on the visible GPU(s) modulo their count, torch.distributed over
    gloo, the exchange staged through the host.  The line is marked invalid: not a measurement."""
    return os.environ.get("FUS_BENCH_REHEARSAL", "0") == "1"


def coll_device(device):
    """Where the tensors of bench.py's own collectives (barrier flags, max-over-ranks time) live."""
    import torch

    return torch.device("cpu") if rehearsal() else device
