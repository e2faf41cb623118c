"""References, bounds and inputs of the three boundary-facet kernels (facet_terms_kernel, facet_source_array_kernel,
facet_source_wave_kernel), shared by the kernels' own tests (tests/test_operators_gpu.py, tests/test_sources_gpu.py,
tests/test_waveform_sources_gpu.py) and tests/test_small_kernels_gpu.py, which runs the same checks at the shapes those do not reach.

    set A:  y[dmA[f][i]] += (v1[f] + v2[f]) detJA[f][i]       v1 = s1 c1 (g_e c1), v2 = s2 c2 (dg_e c2) or absent
    set B:  y[dmB[f][i]] += x[dmB[f][i]] cB[f] detJB[f][i]

Each kernel keeps the reference and the tolerance of its own test:

    facet_terms    ``terms_oracle``: the oracle's mass operator in the kernel's type, applied the reference's way (g and dg filled into
                   vectors); conftest.TOL (rel l2, rel max)
    array source   ``waveform_cpu.facet_reference`` with ``SourceArray.values`` in fp64; ``rel_inf`` <= ``ARRAY_TOL``
    wave source    ``waveform_cpu.facet_reference`` with ``SourceArray.values`` in fp64; conftest.TOL

None of these states a bound per dof, and a whole-vector norm hides a few wrong dofs among 50 000.  ``reference64`` is the fp64
``np.add.at`` on the rounded inputs with, per dof, the number of adds k and |y0| + sum |terms|; ``dof_bound`` is the derivable
(k + 3) eps_T (|y0| + sum |terms|): a term is at most three roundings of (|v1| + |v2|) |detJ| (product, sum, product; x (c detJ) takes
two), each of the k adds rounds a partial sum that is at most the sum of the absolute values.  It holds for facet_terms in both types and
for the source kernels in fp32, where the fp64 evaluation of g_e is exact to the bound's accuracy.  An fp64 source kernel and numpy agree
on g_e to the roundings of their fp64 evaluations, not to 2^-52 of the term: there the bound is widened, per term, by
``evaluation_slack`` (stated against the element's amplitude, since g_e passes through zero).  CPU only; not a test module."""

import numpy as np

ARRAY_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}  # tests/test_sources_gpu.py: rel_inf of the whole vector


def rel_inf(a, b):
    """max |a - b| / max |b|."""
    a, b = (np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64) for x in (a, b))
    assert a.shape == b.shape
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def terms_oracle(oracle_c, y0, g, c1, dg, c2, dA, dmA, field):
    """y0 + the facet terms in the type of ``y0`` by the oracle's mass operator, the reference's way: ``g`` (and, with ``c2``, ``dg``)
    filled into a vector and applied on set A (skipped when it is empty), then ``field = (v, cB, dB, dmB)`` on set B (None: no set B)."""
    dt = y0.dtype
    ref = y0.copy()
    ones = np.ones_like(y0)
    c = np.ascontiguousarray
    if dmA.shape[0]:
        oracle_c.mass_apply((g * ones).astype(dt), c(c1), ref, c(dA), c(dmA))
        if c2 is not None:
            oracle_c.mass_apply((dg * ones).astype(dt), c(c2), ref, c(dA), c(dmA))
    if field is not None and field[3].shape[0]:
        v, cB, dB, dmB = field
        oracle_c.mass_apply(v, c(cB), ref, c(dB), c(dmB))
    return ref


def reference64(y0, v1, v2, dA, dmA, field):
    """(ref, mag, k) per dof in fp64: ``ref`` = y0 + the terms, ``mag`` = |y0| + sum |terms| (|v1| + |v2| for a term of set A), ``k`` the
    number of adds.  ``v1`` / ``v2``: fp64 [nA] (``v2`` None: absent); a facet of set A with v1 = v2 = 0 adds nothing and counts for
    nothing (the source kernels skip it)."""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    ref, mag, k = f(y0).copy(), np.abs(f(y0)), np.zeros(y0.size, dtype=np.int64)
    v2 = np.zeros_like(v1) if v2 is None else v2
    live = (v1 != 0) | (v2 != 0)
    if live.any():
        dm, d = dmA[live].reshape(-1), f(dA)[live]
        np.add.at(ref, dm, ((v1 + v2)[live, None] * d).reshape(-1))
        np.add.at(mag, dm, ((np.abs(v1) + np.abs(v2))[live, None] * np.abs(d)).reshape(-1))
        np.add.at(k, dm, 1)
    if field is not None and field[3].shape[0]:
        x, cB, dB, dmB = field
        t = f(x)[dmB] * (f(cB)[:, None] * f(dB))
        np.add.at(ref, dmB.reshape(-1), t.reshape(-1))
        np.add.at(mag, dmB.reshape(-1), np.abs(t).reshape(-1))
        np.add.at(k, dmB.reshape(-1), 1)
    return ref, mag, k


def dof_bound(mag, k, dtype):
    return (k + 3) * float(np.finfo(dtype).eps) * mag


def evaluation_slack(arr, f0, scale):
    """(eg, edg) per element: how far two correct fp64 evaluations of g_e and dg_e/dt, the kernel's and ``SourceArray.values``, may lie
    apart, in absolute terms.  With a = a_e A:

    analytic   g = a Env cos(theta).  |theta| = |w0 s + phi| stays below 2^7 rad (14 periods and a phase) and either side forms it with
               fewer than 2^3 roundings of 2^-53 (the kernel as pi (2 f0 s + phi / pi)): the two angles differ by at most
               2 x 2^7 x 2^3 x 2^-53 = 2^-42, and so do the two cosines; each window factor (argument below 2^4 rad) likewise by less
               than 2^-42, and a burst has two.  eg = 2^-40 a.  dg = a (Env' cos - Env w0 sin) with |Env'| <= w0: edg = 2^-39 a w0.
    sampled    the cubic Hermite form on exact node times (the tables of the tests use a power-of-two interval).  |h| <= 1 and
               |h'| <= 1.5, so sum |terms| <= 2 (W + dt D) for w and <= 4 (W / dt + D) for dw, W and D the largest |sample| and
               |derivative| of the row; fewer than 8 roundings per term (with or without FMA), two evaluations:
               eg = 2^-48 a (W + dt D), edg = 2^-47 a (W / dt + D)."""
    a = np.abs(np.asarray(arr.amplitude, dtype=np.float64)) * float(scale)
    wf = arr.waveform
    if wf is None:
        return 2.0**-40 * a, 2.0**-39 * a * (2.0 * np.pi * float(f0))
    r = np.maximum(arr.waveform_of_element, 0)
    W, D = np.max(np.abs(wf.samples), axis=1)[r], np.max(np.abs(wf.derivative), axis=1)[r]
    return 2.0**-48 * a * (W + wf.dt * D), 2.0**-47 * a * (W / wf.dt + D)


def facet_sets(rng, dtype, N, nA, nB, ndofs, quiet=None, reserved=0):
    """Random facet sets on ``ndofs`` dofs of which the last ``reserved`` are touched by the facets ``quiet`` (bool [nA]) alone:
    c1 on [0.5, 1.5], c2 on [0, 1e-6] (a derivative constant: dg is of order w0 g), detJ on [0, 1], dofmaps with collisions, x and cB
    standard normal.  -> dict(c1, c2, dA, dmA, x, cB, dB, dmB)."""
    live = ndofs - reserved
    s = dict(c1=rng.random(nA).astype(dtype) + 0.5, c2=(rng.random(nA) * 1e-6).astype(dtype), dA=rng.random((nA, N)).astype(dtype),
             dmA=rng.integers(0, live, (nA, N)).astype(np.int32), x=rng.standard_normal(ndofs).astype(dtype),
             cB=rng.standard_normal(nB).astype(dtype), dB=rng.random((nB, N)).astype(dtype), dmB=rng.integers(0, live, (nB, N)).astype(np.int32))
    if quiet is not None and quiet.any():
        assert reserved > 0
        s["dmA"][quiet] = rng.integers(live, ndofs, (int(quiet.sum()), N)).astype(np.int32)
    return s
