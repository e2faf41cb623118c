"""Point sensors, host side (sensors.py) and the C ABI's argument checks of ``fus_probe_eval_*`` -- no device work here.
The set-up (cell location, reference coordinates, 1-D Lagrange rows) contracted with numpy reproduces
``point_evaluation.eval_function``; points outside a rank are dropped; ``merge`` takes the lowest rank."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import ROOT, pkg


def _contract(setup, u):
    """What the kernel computes, in numpy: sum_ijk Lx[i] Ly[j] Lz[k] u[row[i n^2 + j n + k]]."""
    n = setup.weights.shape[2]
    uc = np.asarray(u, dtype=np.float64)[setup.rows[setup.cell_index]].reshape(-1, n, n, n)
    w = setup.weights
    return np.einsum("mijk,mi,mj,mk->m", uc, w[:, 0], w[:, 1], w[:, 2])


def _bowl(L, N):
    def warp(xg):
        out = xg.copy()
        yy, zz = xg[:, 1] / L - 0.5, xg[:, 2] / L - 0.5
        out[:, 0] = xg[:, 0] + 0.15 * (L / N) * 4 * (yy * yy + zz * zz) * (1.0 - xg[:, 0] / L)
        return out

    return warp


def _mesh(kind, P, L=0.012, cells=(3, 2, 2)):
    boxmesh = pkg("boxmesh")
    if kind == "affine":
        return boxmesh.BoxMesh(P, cells, length=L)
    if kind == "perturbed":
        return boxmesh.BoxMesh(P, cells, length=L, perturb=0.14, seed=2)
    if kind == "bowl":
        return boxmesh.BoxMesh(P, cells, length=L, warp=_bowl(L, cells[0]))
    if kind == "array":  # cells and vertices renumbered at random, handed over as plain arrays
        ad = pkg("dolfinx_adaptor")
        box = boxmesh.BoxMesh(P, cells, length=L, perturb=0.1, seed=4)
        rng = np.random.default_rng(7)
        cperm, vperm = rng.permutation(box.ncells), rng.permutation(box.x_g.shape[0])
        vinv = np.empty_like(vperm)
        vinv[vperm] = np.arange(vperm.size)
        return ad.ArrayMesh(P, box.dofmap[cperm], vinv[box.x_dofs[cperm]], box.x_g[vperm])
    raise ValueError(kind)


def _points(L, cells, rng, m=200, margin=0.0):
    """Random interior points plus cell corners, points on interior cell faces and on the domain boundary."""
    pts = margin + (L - 2 * margin) * rng.random((m, 3))
    h = [L / c for c in cells]
    special = [[0, 0, 0], [L, L, L], [h[0], h[1], h[2]], [h[0], 0.3 * L, 0.6 * L], [0.5 * h[0], h[1], 0.2 * L],
               [0.0, 0.5 * L, 0.5 * L], [L, 0.25 * L, 0.75 * L], [0.3 * L, 0.0, L], [2 * h[0], h[1], 0.0]]
    return np.concatenate([np.asarray(special), pts])


@pytest.mark.parametrize("kind", ["affine", "perturbed", "bowl", "array"])
@pytest.mark.parametrize("P", list(range(2, 11)))
def test_setup_contraction_reproduces_eval_function(P, kind):
    pe, sens = pkg("point_evaluation"), pkg("sensors")
    L, cells = 0.012, (3, 2, 2)
    mesh = _mesh(kind, P, L, cells)
    rng = np.random.default_rng(P)
    pts = _points(L, cells, rng, m=150, margin=0.0 if kind == "affine" else 0.1 * L)
    if kind != "affine":  # the perturbed / warped boundary: keep the points well inside, add the interior cell corners
        pts = pts[np.all((pts > 0.08 * L) & (pts < 0.92 * L), axis=1)]
        xg = np.asarray(mesh.x_g, dtype=np.float64)
        pts = np.concatenate([pts, xg[np.all((xg > 0.05 * L) & (xg < 0.95 * L), axis=1)]])
    u = 1e4 * rng.standard_normal(mesh.ndofs)  # any dof vector: the interpolant is linear in it
    s = sens.sensor_setup(mesh, pts)
    x_eval, cell_eval = pe.compute_eval_params(mesh, pts.T)
    assert s.point_ids.size == len(cell_eval) > 0
    assert np.all(np.diff(s.cells) >= 0)  # device order: sorted by cell
    order = np.argsort(s.point_ids)
    assert np.array_equal(s.points[order], x_eval) and np.array_equal(s.cells[order], np.asarray(cell_eval))
    ref = pe.eval_function(mesh, u, x_eval, cell_eval)
    got = _contract(s, u)[order]
    assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref)))
    assert s.rows.shape == (np.unique(s.cells).size, (P + 1) ** 3)


def test_weights_are_lagrange_rows_at_the_reference_coordinates():
    """Each point's three rows sum to one and reproduce its reference coordinate (degree >= 1 polynomials)."""
    sens, gll = pkg("sensors"), pkg("gll")
    P = 5
    mesh = _mesh("perturbed", P)
    s = sens.sensor_setup(mesh, 0.002 + 0.008 * np.random.default_rng(0).random((60, 3)))
    nodes, _ = gll.gll_points_weights(P)
    assert np.allclose(s.weights.sum(axis=2), 1.0, atol=1e-13)
    xi = s.weights @ nodes  # [m, 3]
    assert np.all((xi >= -1e-13) & (xi <= 1 + 1e-13))


def test_points_outside_the_rank_are_dropped_and_merge_takes_the_lowest_rank():
    boxmesh, sens, pe = pkg("boxmesh"), pkg("sensors"), pkg("point_evaluation")
    P, cells, grid, L = 3, (4, 4, 2), (2, 2, 1), 1.0
    serial = boxmesh.BoxMesh(P, cells, perturb=0.12, seed=5)
    rng = np.random.default_rng(3)
    pts = np.concatenate([0.06 + 0.88 * rng.random((300, 3)), [[0.5, 0.5, 0.5], [0.5, 0.25, 0.3], [5.0, 0.5, 0.5]]])
    f = lambda p: np.sin(3 * p[:, 0]) * np.cos(2 * p[:, 1]) + p[:, 2]  # noqa: E731
    ss = sens.sensor_setup(serial, pts)
    assert ss.point_ids.size == pts.shape[0] - 1 and pts.shape[0] - 1 not in ss.point_ids  # (5, .5, .5) is nowhere
    ref = sens.merge([(ss.point_ids, _contract(ss, f(serial.dof_coordinates())))], pts.shape[0])
    per_rank, owners = [], np.zeros(pts.shape[0], dtype=int)
    for r in range(4):
        m = boxmesh.BoxMesh(P, cells, grid=grid, rank=r, perturb=0.12, seed=5)
        s = sens.sensor_setup(m, pts)
        assert 0 < s.point_ids.size < pts.shape[0] - 1
        owners[s.point_ids] += 1
        vals = _contract(s, f(m.dof_coordinates()))
        per_rank.append((s.point_ids, vals + r))  # tag the rank: merge must take the lowest
    assert np.all(owners[:-1] >= 1) and owners[-1] == 0
    # on the unperturbed partition (0.5, 0.5, 0.5) is a corner of all four blocks: every rank keeps it, rank 0's value wins
    held = [sens.sensor_setup(boxmesh.BoxMesh(P, cells, grid=grid, rank=r), [[0.5, 0.5, 0.5]]) for r in range(4)]
    assert all(h.point_ids.tolist() == [0] for h in held)
    assert sens.merge([(h.point_ids, np.array([10.0 + r])) for r, h in enumerate(held)]).tolist() == [10.0]
    merged = sens.merge(per_rank, pts.shape[0])
    lowest = np.array([next((r for r, (ids, _) in enumerate(per_rank) if k in ids), -1) for k in range(pts.shape[0])])
    assert np.isnan(merged[-1]) and lowest[-1] == -1
    assert np.max(np.abs(merged[:-1] - lowest[:-1] - ref[:-1])) < 1e-12
    # leading axes (a series) are carried through
    two = sens.merge([(ids, np.stack([v, 2 * v])) for ids, v in per_rank], pts.shape[0])
    assert two.shape == (2, pts.shape[0]) and np.allclose(two[0, :-1], merged[:-1])
    # points given in the reference's 3 x m layout are the same points
    assert np.array_equal(sens.sensor_setup(serial, pts.T).point_ids, ss.point_ids)


def test_harmonic_coefficient_table():
    sens = pkg("sensors")
    w, t = 2 * np.pi * 1.1e6, 3.7e-6
    c = sens.harmonic_coefficients((1, 2, 5), w, t)
    assert c.shape == (6,)
    for h, k in enumerate((1, 2, 5)):
        assert c[2 * h] == np.cos(k * w * t) and c[2 * h + 1] == -np.sin(k * w * t)
    # over one period at N equal steps the accumulated sum gives (2 / N)|.| = the amplitude of each harmonic
    N, f0 = 37, 1.1e6
    ts = np.arange(1, N + 1) / (N * f0)
    p = 3.0 * np.cos(2 * np.pi * f0 * ts + 0.4) + 0.5 * np.cos(4 * np.pi * f0 * ts - 1.0) + 0.2
    acc = sum(pi * sens.harmonic_coefficients((1, 2), 2 * np.pi * f0, ti) for pi, ti in zip(p, ts))
    amp = 2.0 / N * np.hypot(acc[0::2], acc[1::2])
    assert np.allclose(amp, [3.0, 0.5], rtol=0, atol=1e-12)
    assert sens.harmonic_coefficients((), w, t).shape == (0,)


@pytest.mark.parametrize("harmonics", [(), (1,), (1, 2, 5)])
def test_coefficient_rows_equal_harmonic_coefficients(harmonics):
    """A planned record reads a row of the table, any other one ``harmonic_coefficients`` of its time: the same factors, bitwise."""
    rec = pkg("recording")
    w = 2 * np.pi * 1.1e6
    rng = np.random.default_rng(17)
    ends = np.cumsum(rng.uniform(0.2e-7, 1.9e-7, 70))  # step ends of 70 steps of random length
    rows = rec.coefficient_rows(harmonics, w, ends)
    assert rows.shape == (70, 2 * len(harmonics)) and rows.flags.c_contiguous
    for row, t in zip(rows, ends):
        assert np.array_equal(row, pkg("sensors").harmonic_coefficients(harmonics, w, t))
        k = np.asarray(harmonics, dtype=np.float64)
        assert np.array_equal(row, np.stack([np.cos(k * w * t), -np.sin(k * w * t)], axis=1).reshape(-1))  # the formula itself


def test_gather_arrays_through_a_bootstrap():
    """What PointSensors.gather and field_monitor.focus send through the communicator's bootstrap comes back as one dict per rank;
    a communicator of ranks driven from one process has none."""
    scat = pkg("scatterer")

    class Boot:  # two ranks; the other one sends what this one does
        size = 2

        def allgather_bytes(self, payload):
            return [payload, payload]

    class InProcess:  # NativeComm(local=...): a handle, no bootstrap
        size, handle, bootstrap = 2, 1, None

    arrays = {"ids": np.arange(3), "values": np.arange(6.0).reshape(2, 3), "max": 2.5}
    every = scat.gather_arrays(Boot(), arrays, "gather", "sensors.merge")
    assert len(every) == 2
    for z in every:
        assert sorted(z) == sorted(arrays) and all(np.array_equal(z[k], arrays[k]) for k in arrays)
        assert z["ids"].dtype == np.int64 and z["max"].shape == ()
    with pytest.raises(ValueError, match=r"^gather: this communicator has no bootstrap \(ranks in one process\): use sensors.merge$"):
        scat.gather_arrays(InProcess(), arrays, "gather", "sensors.merge")
    with pytest.raises(ValueError, match=r"^focus: this communicator has no bootstrap \(ranks in one process\): use merge_focus$"):
        scat.gather_arrays(object(), arrays, "focus", "merge_focus")


def test_probe_argument_validation_precedes_device_work():
    lib = pkg("_lib").load()
    z = C.c_void_p(0)
    one = C.c_void_p(256)  # non-null, never dereferenced: validation fails first
    for fn in (lib.fus_probe_eval_f64, lib.fus_probe_eval_f32):
        def call(u=one, cells=one, npts=4, dm=one, nc=2, w=one, P=4, rec=one, cap=3, slot=0, pmax=one, pmin=one, hre=one, him=one,
                 coef=one, H=2):
            return fn(u, cells, npts, dm, nc, w, P, rec, cap, slot, pmax, pmin, hre, him, coef, H, z)

        assert call(P=11) == -2 and call(P=0) == -2  # unsupported degree
        assert call(npts=-1) == -1 and call(nc=-1) == -1 and call(H=-1) == -1 and call(cap=-1) == -1
        assert call(npts=0, u=z, cells=z, dm=z, w=z) == 0  # no points: no-op, nothing read
        for name in ("u", "cells", "dm", "w"):
            assert call(**{name: z}) == -1, name
        assert call(slot=3) == -1 and call(slot=-1) == -1 and call(cap=0) == -1  # slot outside [0, capacity)
        assert call(coef=z) == -1  # harmonics without their factors
        assert call(hre=one, him=one, coef=z, H=0) == -1  # accumulators without factors
        assert call(hre=z) == -1 and call(him=z) == -1  # H > 0 without an accumulator
        assert call(u=C.c_void_p(258)) == -1 and call(w=C.c_void_p(258)) == -1  # misaligned
        assert call(cells=C.c_void_p(258)) == -1 and call(dm=C.c_void_p(258)) == -1


def test_sensor_setup_of_an_empty_point_set():
    sens = pkg("sensors")
    s = sens.sensor_setup(_mesh("affine", 3), np.zeros((0, 3)))
    assert s.point_ids.size == 0 and s.weights.shape == (0, 3, 4) and s.rows.shape == (0, 64)
    assert sens.merge([(s.point_ids, np.zeros(0))], 5).shape == (5,)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_probe_kernel_builds_without_scratch_at_eight_waves():
    """Every instantiation of the sensor kernel (fp64 / fp32, P = 1 ... 10): no scratch, <= 64 VGPRs (8 waves per SIMD), read
    from hipcc's resource-usage remarks as tests/test_resource_usage.py reads them for the operator kernels."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    hits = {k: v for k, v in ru.parse(ru.cached_remarks()).items() if "probe_eval_kernel" in k}
    assert len(hits) == 20, sorted(hits)
    bad = {k: v for k, v in hits.items() if v["scratch"] != 0 or v["vgpr"] > 64 or v["occupancy"] < 8}
    assert not bad, bad
