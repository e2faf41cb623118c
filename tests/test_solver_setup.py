"""The set-up the three solvers share: the rank agreement on a few floats, the lock-step driver, the one rule for the operator form."""

import types

import numpy as np
import pytest

from conftest import pkg


def test_gather_floats():
    """float64 [size, k] in rank order through a bootstrap (a NativeComm carries its own in ``bootstrap``); no communicator, one rank, a
    handle without a bootstrap: the local row.  ``BioheatSpectral3D._gather`` raises where the rows do not cover every rank."""
    boot = types.SimpleNamespace(size=2, allgather_bytes=lambda blob: [blob, (-np.frombuffer(blob, dtype="<f8")).tobytes()])
    native = lambda size, bootstrap: types.SimpleNamespace(size=size, rank=0, handle=1, bootstrap=bootstrap)  # noqa: E731
    for values in ([1.5, -2.0, 1e-300], []):
        both = [values, [-v for v in values]]
        for comm, rows in ((boot, both), (native(2, boot), both), (None, [values]), (types.SimpleNamespace(size=1), [values]), (native(2, None), [values])):
            every = pkg("scatterer").gather_floats(comm, values)
            assert every.dtype == np.float64 and every.shape == (len(rows), len(values))
            assert np.array_equal(every, np.asarray(rows, dtype=np.float64))
    gather = lambda comm: pkg("solver_base").run_schedule(  # noqa: E731
        pkg("bioheat").BioheatSpectral3D._gather(types.SimpleNamespace(halo=object(), comm=comm), [0.5, 3.0], None, 0))
    assert np.array_equal(gather(native(2, boot)), [[0.5, 3.0], [-0.5, -3.0]])
    for comm in (native(2, None), native(4, boot)):  # ranks of one process; a hosted world of 4 ranks in 2 processes
        with pytest.raises(pkg("_lib").FusGpuError, match="ranks driven from one process share no collective"):
            gather(comm)


def test_run_lockstep():
    trace = []

    def rank(name, nyields, fail=False):
        for k in range(nyields):
            trace.append((name, k))
            yield "posted"
        if fail:
            raise ValueError(f"rank {name} failed")
        return name.upper()

    run_lockstep = pkg("solver_base").run_lockstep
    assert run_lockstep([rank("a", 2), rank("b", 0), rank("c", 3)]) == ["A", "B", "C"]  # values in input order
    assert trace == [("a", 0), ("c", 0), ("a", 1), ("c", 1), ("c", 2)]  # each advanced once before any is advanced twice
    del trace[:]
    with pytest.raises(ValueError, match="^rank b failed$"):
        run_lockstep([rank("a", 3), rank("b", 1, fail=True)])
    assert trace == [("a", 0), ("b", 0), ("a", 1)]  # raised in the second round, after the first generator's turn


MESHES = {"affine-P3": (3, (2, 2, 2), 0.0), "perturbed-P3": (3, (3, 2, 2), 0.12), "perturbed-P2": (2, (3, 2, 2), 0.12)}


@pytest.mark.gpu
@pytest.mark.parametrize("affine", ["auto", False])
@pytest.mark.parametrize("in_kernel_geometry", ["auto", False, True])
@pytest.mark.parametrize("name", list(MESHES))
def test_operator_form_is_decided_once(name, in_kernel_geometry, affine):
    """Affine wins (found under "auto" on a box of affine cells); otherwise G is formed in the kernel from degree 3 under "auto",
    always under True, never under False.  The Westervelt solver's fused stage crosses the same degree threshold."""
    import torch

    torch.cuda.set_device(0)
    P, cells, perturb = MESHES[name]
    mesh = pkg("boxmesh").BoxMesh(P, cells, length=0.01, perturb=perturb, seed=4)
    want_affine = affine == "auto" and perturb == 0.0
    want_kernel = not want_affine and (in_kernel_geometry is True or (in_kernel_geometry == "auto" and P >= 3))
    lin = pkg("linear_solver").LinearSpectral3D(mesh, np.float64, affine=affine, in_kernel_geometry=in_kernel_geometry)
    heat = pkg("bioheat").BioheatSpectral3D(mesh, np.float64, affine=affine, in_kernel_geometry=in_kernel_geometry)
    for s in (lin, heat):  # in the G position: the rows of x_dofs, or the geometric factors
        assert (s.affine, s.in_kernel_geometry) == (want_affine, want_kernel), type(s).__name__
        assert (s.G.dtype, tuple(s.G.shape)) == ((torch.int32, (mesh.ncells, 8)) if want_kernel else (torch.float64, (mesh.ncells, (P + 1) ** 3, 6)))
    assert (lin.G_array is None) == want_kernel and (want_kernel or lin.G_array is lin.G)  # keep_G=False
    if perturb and in_kernel_geometry == "auto" and affine == "auto":
        wave = pkg("nonlinear_solver").WesterveltSpectral3D(mesh, np.float64, fused=True)
        assert wave.in_kernel_geometry == lin.in_kernel_geometry == (P >= 3) and (wave.G is None) == (P >= 3)
