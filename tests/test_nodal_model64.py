"""The fp64 model of the nodal cell operators (tests/nodal_model64.py) on the CPU: what tests/test_nodal_builds_gpu.py takes for granted
about its reference and about the fp32 bar built on it."""

import numpy as np
import pytest

import nodal_cpu
import nodal_model64 as model
import westervelt_nodal_cpu
from conftest import TOL, rel_l2

SHAPE = {1: (5, 4, 7), 3: (4, 3, 3), 4: (3, 3, 3), 5: (5, 3, 1), 10: (7, 1, 1)}


@pytest.mark.parametrize("P", sorted(SHAPE))
def test_the_inputs_are_what_the_gpu_tests_rely_on(P):
    """kappa independent per dof on [0.3, 3] (neighbouring dofs are uncorrelated: a coefficient taken from the dof next door is an O(1)
    error), c4 negative next to a positive c3, y0 a tenth of what the apply adds, everything in the case's type and read-only."""
    geo = model.box(P, SHAPE[P], np.float32)
    s, p = model.stiffness(geo), model.pair(geo)
    for k in (s["kappa"], p["k3"], p["k4"]):
        assert k.dtype == np.float32 and 0.3 * (1 - 1e-6) <= k.min() < 0.5 and 2.0 < k.max() <= 3.0 * (1 + 1e-6)
        lk = np.log(k) - np.log(k).mean()
        assert abs(np.mean(lk[1:] * lk[:-1])) < 0.2 * np.mean(lk * lk)
    assert rel_l2(p["k3"], p["k4"]) > 0.3 and rel_l2(p["u"], p["v"]) > 0.5
    assert p["c4"].max() <= -0.5 and p["c4"].min() >= -1.5 and p["c3"].min() > 0
    for c in (s, p):
        ratio = np.sqrt(np.mean(c["y0"].astype(np.float64) ** 2) / np.mean(c["add"] ** 2))
        assert 0.08 < ratio < 0.12 and c["ref"].dtype == np.float64 and c["cpu32"].dtype == np.float32
        assert not c["ref"].flags.writeable and not c["y0"].flags.writeable
        with pytest.raises(ValueError):
            c["ref"][0] = 0.0


@pytest.mark.parametrize("P", sorted(SHAPE))
def test_the_fp64_case_is_the_cpu_model_of_the_older_tests(P):
    """In fp64 nothing is rounded: the model is ``nodal_cpu.stiffness_apply`` / ``stiffness_pair`` on ``build_problem``'s own G."""
    geo = model.box(P, SHAPE[P], np.float64)
    assert np.array_equal(model.factors64(geo), geo["G"])
    s, p = model.stiffness(geo), model.pair(geo)
    assert s["e_cpu"] is None and s["cpu32"] is None
    y = s["y0"].copy()
    nodal_cpu.stiffness_apply(P, geo["D"], s["x"], geo["cc"], y, geo["G"], geo["dofmap"], s["kappa"])
    assert rel_l2(y, s["ref"]) < 1e-15
    b = p["y0"].copy()
    westervelt_nodal_cpu.stiffness_pair(P, geo["D"], p["u"], p["v"], p["c3"], p["c4"], b, geo["G"], geo["dofmap"], p["k3"], p["k4"])
    assert rel_l2(b, p["ref"]) < 1e-15
    # the two terms of the pair do not cancel: each alone is of the size of the sum
    only_u = np.zeros(geo["ndofs"])
    nodal_cpu.stiffness_apply(P, geo["D"], p["u"], p["c3"], only_u, geo["G"], geo["dofmap"], p["k3"])
    assert 0.2 < np.linalg.norm(only_u) / np.linalg.norm(p["add"]) < 5.0 and rel_l2(only_u, p["add"]) > 0.2


@pytest.mark.parametrize("kind", sorted(model.MODELS))
def test_the_fp32_oracle_is_a_few_units_from_the_model(kind):
    """e_cpu, on which the fp32 bar of the GPU tests is built, is an fp32 evaluation's error: above a quarter of the unit spacing 2^-23
    and below 4 of them in rel l2 (8 in rel max) at every degree and on the colliding dofmap -- so 8 x max(e_cpu, 2^-23) stays at least
    2.5 x below ``TOL`` (l2) and 10 x (max)."""
    u = 2.0**-23
    cases = [model.MODELS[kind](model.box(P, shape, np.float32)) for P, shape in SHAPE.items()] + [model.MODELS[kind](model.colliding(np.float32))]
    for c in cases:
        e2, em = c["e_cpu"]
        print(f"{kind} P={c['P']} {c['ncells']} cells: e_cpu l2 {e2:.3e} max {em:.3e}")
        assert 0.25 * u < e2 < 4 * u and 0.25 * u < em < 8 * u
        tol = TOL[np.dtype(np.float32)]
        assert 8 * max(e2, u) * 2.5 < tol["l2"] and 8 * max(em, u) * 10 < tol["mx"]
