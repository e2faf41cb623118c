"""
The explicit RK4 step a damped oscillator admits (host arithmetic only; numpy, no torch): what ``stable_time_step`` of the two wave
solvers turns its two operator bounds into.

The semi-discrete system ``M v' = -K u - C v`` has, per mode of stiffness ``lambda`` (an eigenvalue of ``M^-1 K``) and damping rate
``d`` (a diagonal entry of ``M^-1 C``), the characteristic roots of ``mu^2 + d mu + lambda = 0``; RK4 keeps such a mode bounded while
``|R(mu dt)| <= 1`` for both roots, ``R(z) = 1 + z + z^2/2 + z^3/6 + z^4/24``.  ``rk4_model_step`` finds the largest such ``dt`` by
bisection: ``2 sqrt 2 / sqrt(lambda)`` without damping, ``2.785... / d`` without stiffness.

In between the model step is NOT monotone.  With ``s = d / sqrt(lambda)`` the damping ratio of a pair and ``g(s)`` its step in units of
``1 / sqrt(lambda)``: ``g`` rises from ``2 sqrt 2`` (a little damping turns the roots into a part of the stability region that reaches
further out), falls to the region's waist ``g(1.08) = 2.6156`` and returns to ``2.785`` at the double root ``s = 2``; beyond it the
fast root ``d/2 + sqrt(d^2/4 - lambda)`` SHRINKS as ``lambda`` grows.  The solvers pair the LARGEST stiffness with the LARGEST damping
rate of the mesh, which belong to different modes in general, so every pair ``(lambda', d')`` below the two maxima may occur:
``rk4_stable_step`` is the smallest model step over all of them.  For a fixed ratio the largest ``lambda'`` is the worst, which leaves
a minimum over the ratio alone: ``min(model(lambda, d), model(lambda, 0), model(0, d))`` and, once ``d / sqrt(lambda)`` is past the
waist, the waist's ``2.6156 / sqrt(lambda)`` -- non-increasing in both arguments by construction.  A model problem, not a proof: ``K``
and ``C`` do not commute.
"""

from __future__ import annotations

import numpy as np

_SLACK = 1.0 + 8.0 * np.finfo(np.float64).eps  # |R| is 1 - O(y^6) near the origin: rounding must not read as growth
_SCAN = 4096


def rk4_growth(z):
    """``|R(z)|`` of the classical RK4 scheme, ``z`` complex (array)."""
    z = np.asarray(z, dtype=np.complex128)
    return np.abs(1.0 + z * (1.0 + z * (0.5 + z * (1.0 / 6.0 + z / 24.0))))


def _roots(lam, d):
    disc = complex(0.25 * d * d - lam) ** 0.5
    return np.array([-0.5 * d + disc, -0.5 * d - disc])


def rk4_model_step(lambda_max, damping_max):
    """The largest ``dt`` up to which ``|R(mu dt)| <= 1`` holds for both roots of ``mu^2 + damping_max mu + lambda_max = 0`` (the first
    crossing, found by a scan and bisection); ``inf`` when both arguments are 0."""
    lam, d = float(lambda_max), float(damping_max)
    if not (lam >= 0.0 and d >= 0.0 and np.isfinite(lam) and np.isfinite(d)):
        raise ValueError(f"rk4_model_step: lambda_max = {lam}, damping_max = {d}: both finite and >= 0")
    mu = _roots(lam, d)
    fastest = float(np.abs(mu).max())
    if fastest == 0.0:
        return np.inf
    stable = lambda dt: bool(np.all(rk4_growth(mu * dt) <= _SLACK))  # noqa: E731
    grid = (8.0 / fastest) * np.arange(1, _SCAN + 1) / _SCAN  # |z| = 8 is far outside the region (|R| > 44 there)
    ok = np.all(rk4_growth(mu[None, :] * grid[:, None]) <= _SLACK, axis=1)
    first = int(np.argmin(ok))  # ok[-1] is False
    lo, hi = (grid[first - 1] if first else 0.0), grid[first]
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if stable(mid):
            lo = mid
        else:
            hi = mid
    return float(lo)


_WAIST = None


def rk4_waist():
    """``(s, g(s))`` at the minimum of the model step over the damping ratio ``s = d / sqrt(lambda)`` of an underdamped pair, in units
    of ``1 / sqrt(lambda)``: where the boundary of RK4's stability region is closest to the origin (found once, by ternary search
    between the two maxima of ``g`` at 0.28 and 1.83)."""
    global _WAIST
    if _WAIST is None:
        lo, hi = 0.5, 1.6
        for _ in range(80):
            a, b = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
            if rk4_model_step(1.0, a) < rk4_model_step(1.0, b):
                hi = b
            else:
                lo = a
        s = 0.5 * (lo + hi)
        _WAIST = (s, rk4_model_step(1.0, s))
    return _WAIST


def rk4_stable_step(lambda_max, damping_max):
    """The smallest ``rk4_model_step`` over every pair of a stiffness up to ``lambda_max`` and a damping rate up to ``damping_max``
    (see the module docstring): equal to the model step on both axes, never above it, non-increasing in both arguments."""
    lam, d = float(lambda_max), float(damping_max)
    step = min(rk4_model_step(lam, d), rk4_model_step(lam, 0.0), rk4_model_step(0.0, d))
    if lam > 0.0:
        s, g = rk4_waist()
        if d > s * np.sqrt(lam):
            step = min(step, g / np.sqrt(lam))
    return step
