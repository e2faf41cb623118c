"""Absorbing sponge layers (sponge.py, csrc/sponge.hpp), the part that needs no GPU: the CPU model of the layer (the stage term of
tests/sponge_cpu.py in the loops of oracle/rk4_oracle.py) and the identity that pins its form, the profile, the layer's dof lists on one and several ranks, the kernel's resource usage and the
argument checks of its entry points."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

import sponge_cpu
from conftest import ROOT, pkg, rel_l2
from oracle import rk4_oracle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_model_without_layer_is_the_oracle_loop_bitwise():
    """sigma == 0 with the term ACTIVE (sigma absent, which the layer's factory turns into zeros, and an explicit array of zeros): both
    loops return the fields of the loop without a term, bit for bit.  This test once guarded a separate restatement of the two loops
    that lived in tests/sponge_cpu.py; that fork is gone (the layer is a ``stage_term`` of the oracle's own loops), and its results
    were compared bit for bit with this model's when it was removed (profiles/oracle_model_refactor.log)."""
    boxmesh = pkg("boxmesh")
    mesh = boxmesh.BoxMesh(2, (3, 2, 2), length=(0.006, 0.004, 0.004), perturb=0.1, seed=1)
    dt = 1.0e-7
    for solve in (rk4_oracle.solve, rk4_oracle.solve_westervelt):
        u_ref, v_ref = solve(mesh, 3, dt)
        assert np.max(np.abs(u_ref)) > 0
        for sigma in (None, np.zeros(mesh.ndofs)):
            u, v = solve(mesh, 3, dt, stage_term=sponge_cpu.layer_term(mesh, sigma))
            assert np.array_equal(_bits(u), _bits(u_ref)) and np.array_equal(_bits(v), _bits(v_ref))


@pytest.fixture(scope="module")
def constant_sigma_runs(oracle_c):
    """Uniform sigma, no facet terms: u(0) a Gaussian, v(0) = -sigma u(0).  Then u = exp(-sigma t) w with w the undamped solution from
    (u(0), 0).  Returns the relative l2 distance between the damped run and exp(-sigma T) times the undamped run at dt and dt / 2
    (the same final time), and at dt with the factor 2 of the v term replaced by 1."""
    boxmesh = pkg("boxmesh")
    P, sigma, c = 3, 2.0e5, 1500.0
    mesh = boxmesh.BoxMesh(P, (6, 2, 2), length=(0.012, 0.004, 0.004), perturb=0.1, seed=2)
    X = mesh.dof_coordinates()
    u_init = np.exp(-((X[:, 0] - 0.006) ** 2) / 0.0015**2)  # a plane pulse of width 1.5 mm centred at x = 6 mm
    dt = 0.65 * (np.sqrt(3) * 0.002) / (c * P**2)
    kw = dict(facets=False, oracle_c=oracle_c)

    def distance(steps, h, **more):
        T = steps * h
        ud, _ = rk4_oracle.solve(mesh, steps, h, stage_term=sponge_cpu.layer_term(mesh, sigma, **more), u=u_init, v=-sigma * u_init, **kw)
        uw, _ = rk4_oracle.solve(mesh, steps, h, u=u_init, v=0 * u_init, **kw)
        return rel_l2(ud, np.exp(-sigma * T) * uw)

    return dict(dt=distance(16, dt), half=distance(32, dt / 2), factor_one=distance(16, dt, cv_factor=1.0))


def test_constant_sigma_damps_without_changing_the_wave(constant_sigma_runs):
    """Measured: 3.71e-4 at dt, 2.73e-5 at dt / 2 (ratio 13.6: fourth order gives 16); 0.366 with the factor 1 (and, not asserted,
    0.127 without the sigma^2 term, 0.260 with its sign wrong)."""
    d = constant_sigma_runs
    print(d)
    assert d["dt"] < 1e-2
    assert d["half"] <= d["dt"] / 8
    assert d["factor_one"] > 0.1


# ---- the profile -------------------------------------------------------------------------------------------------------------------
def test_box_profile():
    sp = pkg("sponge")
    lo, hi, L, c = (0.0, 0.0, 0.0), (0.12, 0.06, 0.06), 0.01, 1500.0
    sig = sp.box_profile(lo, hi, L, sp.LATERAL, c, order=2, reflection=1e-4)
    smax = -(2 + 1) * c * np.log(1e-4) / (2 * L)
    assert abs(sp.sigma_max_of(L, c, 2, 1e-4) - smax) < 1e-9 * smax
    rng = np.random.default_rng(0)
    pts = rng.uniform(lo, hi, size=(4000, 3))
    s = sig(pts)
    inside = np.all((pts[:, 1:] >= L) & (pts[:, 1:] <= np.asarray(hi)[1:] - L), axis=1)
    assert inside.any() and (~inside).any()
    assert np.all(s[inside] == 0.0) and np.all(s[~inside] > 0.0) and np.all(s <= smax * (1 + 1e-15))
    # x is no chosen face: nothing depends on it, and the x faces themselves are free of the layer
    assert sig(np.array([[0.0, 0.03, 0.03], [0.12, 0.03, 0.03]])).tolist() == [0.0, 0.0]
    # non-decreasing in depth, sigma_max on the face, zero at the layer's edge
    y = np.linspace(L, 0.0, 101)
    line = sig(np.stack([np.full_like(y, 0.05), y, np.full_like(y, 0.03)], axis=1))
    assert np.all(np.diff(line) >= 0) and line[0] == 0.0 and abs(line[-1] - smax) < 1e-9 * smax
    assert abs(line[50] - smax * 0.25) < 1e-9 * smax  # order 2 at half depth
    # overlap: the maximum of the two faces' values
    p = np.array([[0.05, 0.002, 0.007]])
    one = lambda f: sp.box_profile(lo, hi, L, (f,), c)(p)[0]  # noqa: E731
    assert one("-y") > one("-z") > 0 and sig(p)[0] == one("-y")
    # the upper faces mirror the lower ones; a thickness per axis
    assert abs(sig(np.array([[0.05, 0.06 - 0.002, 0.03]]))[0] - one("-y")) < 1e-9 * smax
    per_axis = sp.box_profile(lo, hi, (0.01, 0.02, 0.005), ("+y", "-z"), c)
    assert abs(per_axis(np.array([[0.0, 0.06, 0.03]]))[0] - sp.sigma_max_of(0.02, c)) < 1e-9 * smax
    assert abs(per_axis(np.array([[0.0, 0.03, 0.0]]))[0] - sp.sigma_max_of(0.005, c)) < 1e-9 * smax
    for bad in (dict(faces=("-w",)), dict(thickness=0.0), dict(thickness=0.07), dict(reflection=1.5), dict(order=-1)):
        kw = dict(lower=lo, upper=hi, thickness=L, faces=sp.LATERAL, speed_of_sound=c)
        kw.update(bad)
        with pytest.raises(ValueError):
            sp.box_profile(**kw)


# ---- the layer's dof list ----------------------------------------------------------------------------------------------------------
def _layer(sp, length, cells, ncell_layer=1):
    h = [length[a] / cells[a] for a in range(3)]
    return sp.box_profile((0, 0, 0), length, (h[0], ncell_layer * h[1], ncell_layer * h[2]), sp.LATERAL, 1500.0)


def test_build_lists_the_owned_layer_dofs():
    boxmesh, sp = pkg("boxmesh"), pkg("sponge")
    P, cells, length = 3, (4, 4, 4), (0.012, 0.008, 0.008)
    mesh = boxmesh.BoxMesh(P, cells, length=length)
    sigma = _layer(sp, length, cells)
    layer = sp.SpongeLayer(sigma)
    idx, sig = layer.build(mesh)
    full = sigma(mesh.dof_coordinates()[: mesh.nlocal])
    assert idx.dtype == np.int32 and sig.dtype == np.float64 and idx.size == sig.size
    assert np.all(np.diff(idx) > 0) and idx.min() >= 0 and idx.max() < mesh.nlocal
    assert np.array_equal(idx, np.nonzero(full > 0)[0]) and np.array_equal(sig, full[idx])
    assert 0 < idx.size < mesh.nlocal and layer.sigma_max == sig.max()
    # one cell on each lateral face: P dof planes per face (the face itself included, the layer's edge plane not)
    ny = P * cells[1] + 1
    assert idx.size == (P * cells[0] + 1) * (ny * ny - (ny - 2 * P) ** 2)
    # the array form gives the same list
    idx2, sig2 = sp.SpongeLayer(full).build(mesh)
    assert np.array_equal(idx2, idx) and np.array_equal(sig2, sig)
    # an empty layer
    empty = sp.SpongeLayer(np.zeros(mesh.nlocal))
    assert empty.build(mesh)[0].size == 0 and empty.sigma_max == 0.0


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 2, 2)])
def test_build_partitions_the_single_rank_list(grid):
    """Every global dof of the single-rank list is in exactly one rank's list, with the same sigma, and no other dof is in any."""
    boxmesh, sp = pkg("boxmesh"), pkg("sponge")
    P, cells, length = 3, (4, 4, 4), (0.012, 0.008, 0.008)
    sigma = _layer(sp, length, cells)
    serial = boxmesh.BoxMesh(P, cells, length=length)
    idx, sig = sp.SpongeLayer(sigma).build(serial)
    want = np.zeros(serial.ndofs)
    want[serial.global_lexicographic_ids()[idx]] = sig
    seen, got = np.zeros(serial.ndofs, dtype=int), np.zeros(serial.ndofs)
    layer = sp.SpongeLayer(sigma)  # one object for every rank, as a driver of several in-process ranks would pass it
    for r in range(int(np.prod(grid))):
        m = boxmesh.BoxMesh(P, cells, grid=grid, rank=r, length=length, ghost_order=3)
        ri, rs = layer.build(m)
        assert np.all(np.diff(ri) > 0) and (ri.size == 0 or ri.max() < m.nlocal)
        lex = m.global_lexicographic_ids()[ri]
        seen[lex] += 1
        got[lex] = rs
    assert np.array_equal(seen, (want > 0).astype(int))
    assert np.allclose(got, want, rtol=1e-12, atol=0.0)


def test_bad_sigma_raises():
    boxmesh, sp = pkg("boxmesh"), pkg("sponge")
    mesh = boxmesh.BoxMesh(2, (2, 2, 2))
    good = np.zeros(mesh.nlocal)
    for bad_value in (-1.0, np.nan, np.inf):
        bad = good.copy()
        bad[3] = bad_value
        with pytest.raises(ValueError):
            sp.SpongeLayer(bad)
        with pytest.raises(ValueError):
            sp.SpongeLayer(lambda xyz, b=bad: b[: xyz.shape[0]]).build(mesh)
    with pytest.raises(ValueError):
        sp.SpongeLayer(good[:-1]).build(mesh)  # not one value per owned dof
    with pytest.raises(ValueError):
        sp.SpongeLayer(np.zeros((2, 2)))


# ---- the kernel, without a GPU -----------------------------------------------------------------------------------------------------
def test_sponge_kernel_resource_usage():
    """sponge_terms_kernel (fp64 / fp32 x the three streaming flavours): no scratch, no LDS, at most 64 vector registers (8 waves per
    SIMD), from hipcc's resource-usage remarks as tests/test_sensors.py reads them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    hits = {k: v for k, v in ru.parse(ru.cached_remarks()).items() if "sponge_terms_kernel" in k}
    assert len(hits) == 6, sorted(hits)
    bad = {k: v for k, v in hits.items() if v["scratch"] != 0 or v["lds"] != 0 or v["vgpr"] > 64 or v["occupancy"] < 8}
    assert not bad, bad


@pytest.mark.parametrize("name", ["fus_sponge_terms_f64", "fus_sponge_terms_f32"])
def test_argument_validation_precedes_device_work(name):
    """Pointers that are never dereferenced (as tests/test_abi.py): every check fails, or passes, before any device work."""
    f = getattr(pkg("_lib").load(), name)
    z, one = C.c_void_p(0), C.c_void_p(256)
    assert f(one, one, one, one, one, one, -1, z) == -1  # negative size
    assert f(z, z, z, z, z, z, 0, z) == 0  # an empty list: a no-op whatever the pointers
    assert f(one, one, one, one, one, one, 0, z) == 0
    for k in range(6):  # each pointer null in turn
        args = [one] * 6
        args[k] = z
        assert f(*args, 5, z) == -1
    assert f(one, one, one, C.c_void_p(258), one, one, 5, z) == -1  # idx not 4-byte aligned
    assert f(C.c_void_p(257), one, one, one, one, one, 5, z) == -1  # y not aligned to its type
    assert pkg("_lib").load().fus_abi_version() == 3  # the new entry points are additive
