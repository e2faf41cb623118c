"""The step bound and the energy of the wave solvers without a GPU: RK4's stability polynomial and the bisection on it, the bound at
exact eigenvalues against the true limit of dense first-order matrices (tests/wave_energy_cpu.py), and the CPU model of the runs
tests/test_energy_gpu.py repeats on the device."""
import numpy as np
import pytest

import wave_energy_cpu as we
from conftest import pkg

REAL_AXIS = float(max(r.real for r in np.roots([1.0, -4.0, 12.0, -24.0]) if abs(r.imag) < 1e-12))  # R(-x) = 1: x^3 - 4x^2 + 12x - 24 = 0


def test_polynomial_closed_forms():
    """Without damping the roots are +-i sqrt(lambda) and |R(iy)|^2 = 1 - y^6/72 + y^8/576 <= 1 up to y = 2 sqrt 2; without stiffness
    the roots are 0 and -d and R(-x) <= 1 up to the real root of x^3 - 4x^2 + 12x - 24."""
    st = pkg("stability")
    assert abs(REAL_AXIS - 2.785293563405282) < 1e-12
    for lam in (1e-6, 0.37, 1.0, 4.0e9, 7.7e15):
        for fn in (st.rk4_model_step, st.rk4_stable_step):
            assert abs(fn(lam, 0.0) * np.sqrt(lam) / (2.0 * np.sqrt(2.0)) - 1.0) <= 1e-12, (fn.__name__, lam)
    for d in (1e-6, 0.37, 1.0, 4.0e5, 7.7e9):
        for fn in (st.rk4_model_step, st.rk4_stable_step):
            assert abs(fn(0.0, d) * d / REAL_AXIS - 1.0) <= 1e-12, (fn.__name__, d)
    assert st.rk4_model_step(0.0, 0.0) == np.inf
    assert abs(st.rk4_growth(2.0j * np.sqrt(2.0)) - 1.0) < 1e-13 and abs(st.rk4_growth(-REAL_AXIS) - 1.0) < 1e-13  # (np.roots: ~1e-14)
    with pytest.raises(ValueError):
        st.rk4_model_step(-1.0, 0.0)


def test_stable_step_is_monotone_and_below_the_model():
    """Non-increasing in both arguments (to the last bits of the bisection), and never above the model step of ANY pair below the
    two bounds: the model step itself is not monotone (a pair at the waist of the region, an overdamped pair)."""
    st = pkg("stability")
    lams, ds = 10.0 ** np.linspace(-2, 2, 21), np.concatenate([[0.0], 10.0 ** np.linspace(-2, 2, 21)])
    F = np.array([[st.rk4_stable_step(lam, d) for d in ds] for lam in lams])
    assert np.all(F[1:, :] <= F[:-1, :] * (1 + 1e-12)) and np.all(F[:, 1:] <= F[:, :-1] * (1 + 1e-12))
    M = np.array([[st.rk4_model_step(lam, d) for d in ds] for lam in lams])
    assert np.any(M[:, 1:] > M[:, :-1] * 1.001) and np.any(M[1:, :] > M[:-1, :] * 1.001)  # the reason for the envelope
    for i in range(len(lams)):
        for j in range(len(ds)):
            assert F[i, j] <= M[: i + 1, : j + 1].min() * (1 + 1e-12)
    s, g = st.rk4_waist()
    assert 1.0 < s < 1.2 and 2.61 < g < 2.62 and g <= min(st.rk4_model_step(1.0, x) for x in np.linspace(0.0, 2.0, 81)) * (1 + 1e-9)


@pytest.mark.parametrize("name", ["linear", "sponge", "westervelt"])
def test_bound_at_exact_eigenvalues_is_below_the_true_limit(name):
    """0.8 x the formula at the exact lambda_max and damping_max <= dt*, the largest dt at which every eigenvalue of the dense
    first-order matrix stays in RK4's stability region.  formula(1) / dt* comes out as 0.912 (linear: the absorbing facets' rate is about
    sqrt(lambda_max), the pair sits at the waist of the region), 0.743 (sponge) and 0.718 (westervelt); DESIGN 3.17."""
    cfg = we.configuration(name)
    lam, dmax, limit, formula = cfg.lambda_max(), cfg.damping_max(), cfg.true_limit(), cfg.formula(1.0)
    print(f"{name}: lambda_max {lam:.6e}, damping_max {dmax:.6e}, sqrt(lambda) {np.sqrt(lam):.4e}, formula(1) {formula:.6e}, dt* {limit:.6e}, "
          f"formula(1)/dt* {formula / limit:.4f}")
    assert 0.8 * formula <= limit
    if name == "sponge":  # the damping binds: the undamped step alone would be three times as long
        assert formula < 0.5 * 2.0 * np.sqrt(2.0) / np.sqrt(lam)
    if name == "westervelt":  # the diffusivity matters: its rate is most of the damping bound and shortens the step
        assert np.max(cfg.delta / cfg.c**2) * lam > 0.9 * dmax - np.max(cfg.facet / cfg.m) and formula < 2.0 * np.sqrt(2.0) / np.sqrt(lam)


def test_true_limit_is_a_limit():
    """The dense limit separates decay from growth in the CPU model's own time loop (the linear configuration)."""
    cfg = we.configuration("linear")
    u0, v0 = we.smooth_state(cfg.mesh, seed=1)
    limit = cfg.true_limit()
    energy = lambda s: sum(cfg.energy(*s))  # noqa: E731
    below, above = cfg.run(u0, v0, 60, 0.98 * limit), cfg.run(u0, v0, 60, 1.1 * limit)
    assert energy(below[-1]) <= energy((u0, v0)) and energy(above[-1]) > 10.0 * energy((u0, v0))


def decay_case():
    """The decay run of tests/test_energy_gpu.py: P = 4 on (2, 2, 2) perturbed cells, two materials, source off, a pulse in the middle
    of the box, 40 steps at half the bound."""
    mesh = we.box(P=4, cells=(2, 2, 2), perturb=0.1, seed=5)
    cfg = we.Dense(mesh, "linear", *we.two_materials(mesh))
    return cfg, we.pulse(mesh), np.zeros(mesh.ndofs), 40, 0.5 * cfg.formula(1.0)


def test_decay_run_loses_energy_every_step():
    cfg, u0, v0, nsteps, dt = decay_case()
    E = np.array([sum(cfg.energy(u0, v0))] + [sum(cfg.energy(*s)) for s in cfg.run(u0, v0, nsteps, dt)])
    print("decay: E_0", E[0], "E_last / E_0", E[-1] / E[0], "largest step ratio", float(np.max(E[1:] / E[:-1])))
    assert np.all(E[1:] <= E[:-1]) and E[-1] < E[0]


def blow_up_case():
    """The guard's run: the linear configuration from a smooth state at 1.5 x the bound, limit 1e6 x the initial amplitude."""
    cfg = we.configuration("linear")
    u0, v0 = we.smooth_state(cfg.mesh, seed=2)
    return cfg, u0, v0, 1e6 * float(np.abs(u0).max())


def steps_to_exceed(cfg, u0, v0, dt, limit, most):
    for k, (u, _) in enumerate(cfg.run(u0, v0, most, dt), start=1):
        if not np.all(np.isfinite(u)) or np.abs(u).max() > limit:
            return k
    return None


def test_blow_up_run_is_bounded_in_steps():
    cfg, u0, v0, limit = blow_up_case()
    k = steps_to_exceed(cfg, u0, v0, 1.5 * cfg.formula(1.0), limit, 400)
    print("1.5 x the bound: max |u| exceeds 1e6 x the initial amplitude after", k, "steps")
    assert k is not None and k <= 200
    assert steps_to_exceed(cfg, u0, v0, 0.8 * cfg.formula(1.0), limit, 200) is None
