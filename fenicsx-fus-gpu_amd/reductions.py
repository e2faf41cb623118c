"""
Reductions over device vectors (``fus_reduce_terms_*``, csrc/reduce.hpp): two sums of products, the largest finite magnitude and the
number of non-finite entries of the first ``n`` entries, in one streaming pass and a one-workgroup finish launch.

    red = Reducer()
    row = red.terms(sum0=(v, v, m), sum1=(u, y, None), x=u, n=nlocal)   # device row of 4 doubles, no host sync
    d = red.dot(w, v, mc, n=nlocal)                                     # one sync
    amax, bad = red.absmax(u, n=nlocal)                                 # one sync

The order of the additions is fixed (no atomics, no counters): two calls on the same data give the same bits, and the launches can be
captured into a hipGraph and replayed as they stand.  There is no CPU fallback.
"""

from __future__ import annotations

import torch

from . import _lib


class Reducer:
    """A workspace (grown on demand) and a device result row for ``fus_reduce_terms_*`` on ``device`` (default: the current one).
    The launches go to the current stream; a ``Reducer`` serves one stream at a time."""

    def __init__(self, device=None):
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.dev.type != "cuda":
            raise _lib.FusGpuError(f"Reducer: device {self.dev}; the reductions only run on the GPU (no CPU fallback)")
        self._lib = _lib.load()
        self._ws = torch.empty(0, dtype=torch.float64, device=self.dev)
        self._ws_n = -1  # the largest n the workspace has been sized for
        self._out = torch.zeros(4, dtype=torch.float64, device=self.dev)

    def _workspace(self, n):
        if n > self._ws_n:
            nbytes = self._lib.fus_reduce_workspace_bytes(n)
            if nbytes < 0:
                _lib.check(int(nbytes), "fus_reduce_workspace_bytes")
            if nbytes > self._ws.numel() * 8:
                self._ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.dev)
            self._ws_n = n
        return self._ws

    def terms(self, sum0=None, sum1=None, x=None, n=None, out=None):
        """``[sum a0 b0 c0, sum a1 b1 c1, max |x| over the finite entries, number of non-finite entries of x]`` over the first ``n``
        entries (default: the length of the shortest operand) as a device row of 4 doubles: this ``Reducer``'s own row, valid until its
        next call, or ``out`` (a contiguous view of 4 doubles on the device, e.g. a row of a recorder's series).  ``sum0`` / ``sum1``:
        ``(a, b, c)`` with ``c`` a weight or ``None`` (then 1), or ``None`` (the sum is 0); ``x``: a vector or ``None`` (0 and 0).
        All operands share one dtype, float32 or float64; products and sums are formed in double either way.  No host sync."""
        operands, names = [], ("a", "b", "c")
        for k, term in enumerate((sum0, sum1)):
            if term is None:
                operands += [None, None, None]
                continue
            if len(term) != 3 or term[0] is None or term[1] is None:
                raise ValueError(f"sum{k}: (a, b, c) with c a weight or None, or None for no sum")
            operands += list(term)
        operands.append(x)
        given = [(t, f"sum{i // 3}[{names[i % 3]}]" if i < 6 else "x") for i, t in enumerate(operands) if t is not None]
        if not given:
            raise ValueError("terms: neither a sum nor x given")
        dtype = getattr(given[0][0], "dtype", None)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{given[0][1]}: expected a float32 or float64 device array, got {dtype or type(given[0][0]).__name__}")
        for t, name in given:
            _lib.require_device_tensor(t, dtype, name)
            if t.device != self.dev:
                raise _lib.FusGpuError(f"{name}: tensor is on {t.device}, this Reducer on {self.dev}")
        shortest = min(t.numel() for t, _ in given)
        n = shortest if n is None else int(n)
        if n < 0 or n > shortest:
            raise ValueError(f"n = {n}: the shortest operand holds {shortest} entries")
        if out is None:
            out = self._out
        else:
            _lib.require_device_tensor(out, torch.float64, "out")
            if out.numel() != 4 or out.device != self.dev:
                raise ValueError(f"out: a view of 4 doubles on {self.dev}")
        fn = getattr(self._lib, f"fus_reduce_terms_{_lib.suffix(dtype)}")
        ptrs = [0 if t is None else t.data_ptr() for t in operands]
        _lib.check(fn(*ptrs, n, out.data_ptr(), self._workspace(n).data_ptr(), _lib.stream_ptr()), "fus_reduce_terms")
        return out

    def dot(self, a, b, w=None, n=None) -> float:
        """``sum a b w`` (``w`` None: ``sum a b``) over the first ``n`` entries, on the host: one sync."""
        return float(self.terms(sum0=(a, b, w), n=n)[0].item())

    def absmax(self, x, n=None):
        """``(max |x| over the finite entries, number of non-finite entries)`` of the first ``n`` entries, on the host: one sync."""
        row = self.terms(x=x, n=n).tolist()
        return float(row[2]), int(row[3])
