"""The launch shape of ``fus_reduce_terms_*`` (csrc/reduce.hpp, csrc/stream_shape.hpp) as plain Python, and what follows from it: the
grid of every piece, the number of workspace rows, and the depth of the addition tree a term passes through -- the constant of the
rounding bound of tests/test_reduce_gpu.py.  tests/test_reduce.py asserts the constants below against the header text."""
import math

import numpy as np

BLOCK = 256  # threads of a workgroup (__launch_bounds__(256))
WAVE = 64  # lanes a __shfl_down tree covers: offsets 32, 16, 8, 4, 2, 1
WAVES = BLOCK // WAVE  # partials thread 0 adds through LDS
GRID_CAP = 2048  # kStreamGridCap
LAUNCH_DOFS = 1 << 27  # kLaunchDofs
STREAM_BYTES = 24 << 20  # kStreamBytes
SLOTS = 4  # kReduceSlots


def width(itemsize, aligned):
    """Entries per thread and trip: one 16-byte access per operand, or the scalar build."""
    return 16 // itemsize if aligned else 1


def pieces(n):
    """``(at, len)`` of for_each_piece(n, kLaunchDofs)."""
    return [(at, min(LAUNCH_DOFS, n - at)) for at in range(0, n, LAUNCH_DOFS)]


def blocks(length, w):
    """stream_blocks(len, w, kStreamGridCap)"""
    return min(((length + w - 1) // w + BLOCK - 1) // BLOCK, GRID_CAP)


def rows(n, itemsize, aligned):
    """Workspace rows a call writes: one per workgroup of every piece."""
    return sum(blocks(length, width(itemsize, aligned)) for _, length in pieces(n))


def workspace_bytes(n):
    """fus_reduce_workspace_bytes: the rows of the scalar build (the most), never 0."""
    return max(rows(n, 8, False), 1) * SLOTS * 8


def chain(length, w):
    """The most entries one thread of a piece adds serially: its trips of w entries and one entry of the scalar tail."""
    if length == 0:
        return 0
    sweep = blocks(length, w) * BLOCK * w
    full = length - length % w
    return -(-full // sweep) * w + (1 if w > 1 and length % w else 0)


def tree_levels():
    """Additions on the way from a thread's partial to its block's: the shuffle tree, then the other waves' partials."""
    return int(math.log2(WAVE)) + (WAVES - 1)


def depth(n, itemsize, aligned):
    """Roundings between an exact term a b c and the result, at most: two for the product (a b, then times c), one per addition of
    the thread's chain, the block tree, the finish kernel's chain over the rows (thread t: rows t, t + 256, ...) and its tree.  The
    first-order bound depth u sum|t_i| neglects the factor 1 / (1 - depth u): one more unit of u covers it for every depth below
    2^26, and the half ulp of the correctly rounded reference sum as well."""
    w = width(itemsize, aligned)
    longest = max((chain(length, w) for _, length in pieces(n)), default=0)
    finish = -(-rows(n, itemsize, aligned) // BLOCK)
    return 2 + longest + tree_levels() + finish + tree_levels() + 1


def short_mantissa(values, bits=17):
    """``values`` as float32 with the mantissa cut to ``bits`` bits: a product of three such numbers has at most 3 * 17 = 51 bits and
    is exact in double, so math.fsum of the double products is the correctly rounded exact sum, for float and double inputs alike."""
    a = np.ascontiguousarray(values, dtype=np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFFFFFF << (24 - bits) & 0xFFFFFFFF)).view(np.float32)


def expected(a0=None, b0=None, c0=None, a1=None, b1=None, c1=None, x=None):
    """``(sums, abs_sums, absmax, nonfinite)`` of host arrays in double: the two sums by math.fsum (exact where the products are),
    ``abs_sums`` = sum |t_i| of each."""
    sums, mags = [], []
    for a, b, c in ((a0, b0, c0), (a1, b1, c1)):
        if a is None:
            sums.append(0.0)
            mags.append(0.0)
            continue
        t = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
        if c is not None:
            t = t * np.asarray(c, dtype=np.float64)
        sums.append(math.fsum(t.tolist()))
        mags.append(math.fsum(np.abs(t).tolist()))
    if x is None:
        return sums, mags, 0.0, 0
    xd = np.asarray(x, dtype=np.float64)
    ok = np.isfinite(xd)
    return sums, mags, float(np.abs(xd[ok]).max()) if ok.any() else 0.0, int((~ok).sum())
