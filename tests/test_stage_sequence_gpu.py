"""Which C entry points one ``rk4`` step calls, in which order, pinned on the GPU with a forwarding proxy for the library: both wave
solvers, the fused stage and the reference launch sequence, with and without a phased-array source, and with a sponge layer, a point
source and relaxation mechanisms together -- each with sensors, receivers and a monitor recording the step.  The lists below were
recorded from the commit before the solvers' attachments were gathered into one source object and one list of stage terms; they are
the specification of that change and of every later one that is meant to leave the launches alone.  ``rk4_graph`` is held against
``rk4`` on the same mesh."""

import numpy as np
import pytest

from conftest import pkg, rel_l2

pytestmark = pytest.mark.gpu

F0, C0 = 0.5e6, 1500.0
LENGTH = (0.006, 0.0045, 0.0045)


class _Forward:
    """The loaded library with every ``fus_*`` entry recorded by name (while ``on``) on its way to the real function: the recording
    idea of ``_Library`` in tests/test_operator_routes.py, with the call going through."""

    def __init__(self, real):
        self.real, self.names, self.on = real, [], False

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("fus_"):
            return fn

        def call(*args):
            if self.on:
                self.names.append(name)
            return fn(*args)

        return call


@pytest.fixture
def library(monkeypatch):
    """The proxy in the place of ``_lib.load()``'s library, before anything is constructed (``PointSensors`` and ``FieldMonitor``
    look their entry point up in the constructor)."""
    import torch

    torch.cuda.set_device(0)
    lib_mod = pkg("_lib")
    proxy = _Forward(lib_mod.load())
    monkeypatch.setattr(lib_mod, "_lib", proxy)
    return proxy


def _mesh():
    """P = 2 on 4 x 3 x 3 perturbed cells: the smallest on which a one-cell lateral layer is non-empty and leaves interior dofs, and
    an interior point source and a sensor point lie in different cells."""
    boxmesh, ls = pkg("boxmesh"), pkg("linear_solver")
    mesh = boxmesh.BoxMesh(2, (4, 3, 3), length=LENGTH, perturb=0.1, seed=5)
    h = ls.time_step_parameters(mesh, 2, C0, F0, LENGTH[0])
    return mesh, ls.snap_time_step(h, 2, C0, F0, LENGTH[0])[0]


def _attachments(mesh, extras):
    src, sp, rx = pkg("sources"), pkg("sponge"), pkg("relaxation")
    if extras == "plain":
        return {}
    if extras == "array":
        grid = src.grid_elements(2, 1, (0.0, LENGTH[1]), (0.0, LENGTH[2]))
        return dict(source=src.SourceArray(grid, amplitude=[1.0, 0.7], phase=[0.0, 0.9], n_elements=2))
    hy, hz = LENGTH[1] / 3, LENGTH[2] / 3
    sigma = sp.box_profile((0.0, 0.0, 0.0), LENGTH, (LENGTH[0], hy, hz), sp.LATERAL, C0)
    point = src.PointSources(np.array([[0.41, 0.57, 0.36]]) * np.asarray(LENGTH), amplitude=0.05)  # cell (1, 1, 1)
    return dict(sponge=sp.SpongeLayer(sigma), point_source=point, relaxation=rx.RelaxationAbsorption([8e-7, 3e-7], [0.06, 0.03]))


def _solver(which, mesh, fused, extras):
    kw = _attachments(mesh, extras)
    if which == "linear":
        return pkg("linear_solver").LinearSpectral3D(mesh, np.float64, fused=fused, **kw)
    return pkg("nonlinear_solver").WesterveltSpectral3D(mesh, np.float64, speed_of_sound=C0, source_frequency=F0, fused=fused, **kw)


def _recorders(mesh, s):
    sens, rxm, fm, src = pkg("sensors"), pkg("receivers"), pkg("field_monitor"), pkg("sources")
    pts = np.array([[0.68, 0.31, 0.62], [0.9, 0.5, 0.5]]) * np.asarray(LENGTH)  # cells (2, 0, 1) and (3, 1, 1)
    grid = src.grid_elements(2, 1, (0.0, LENGTH[1]), (0.0, LENGTH[2]))
    return dict(sensors=sens.PointSensors(mesh, pts, np.float64, capacity=2, peak=True, harmonics=(1,), frequency=F0),
                receivers=rxm.ElementReceivers(mesh, grid, np.float64, capacity=2, harmonics=(1,), frequency=F0, n_elements=2),
                monitor=fm.FieldMonitor(s.nlocal, np.float64, peak=True, mean_square=("u", "v"), harmonics=(1,), frequency=F0))


def _words(names):
    """The entry names without the ``fus_`` / ``_f64`` every one of them carries."""
    assert all(n.startswith("fus_") for n in names)
    return [n[4:-4] if n.endswith("_f64") else n[4:] for n in names]


# one rk4 step (the second of a run: the first has built the batch plans) with sensors, receivers and a monitor, recorded on the
# parent of the change described above
EXPECTED = {
    "linear-fused-plain": """
        fill copy copy stiffness_apply_planned facet_terms rk4_stage stiffness_apply_planned facet_terms
        rk4_stage stiffness_apply_planned facet_terms rk4_stage stiffness_apply_planned facet_terms rk4_stage probe_eval
        element_receive field_accumulate copy copy
    """.split(),
    "linear-fused-array": """
        fill copy copy stiffness_apply_planned facet_source_array rk4_stage stiffness_apply_planned facet_source_array
        rk4_stage stiffness_apply_planned facet_source_array rk4_stage stiffness_apply_planned facet_source_array rk4_stage probe_eval
        element_receive field_accumulate copy copy
    """.split(),
    "linear-fused-sponge-points-relaxation": """
        fill copy copy stiffness_apply_planned facet_terms sponge_terms point_source relax_stage
        rk4_stage stiffness_apply_planned facet_terms sponge_terms point_source relax_stage rk4_stage stiffness_apply_planned
        facet_terms sponge_terms point_source relax_stage rk4_stage stiffness_apply_planned facet_terms sponge_terms
        point_source rk4_stage relax_stage probe_eval element_receive field_accumulate copy copy
    """.split(),
    "linear-reference-sequence-plain": """
        copy copy copy copy axpy axpy copy fill
        copy copy fill stiffness_apply_planned mass_apply mass_apply pointwise_divide axpy
        axpy copy copy axpy axpy copy fill copy
        copy fill stiffness_apply_planned mass_apply mass_apply pointwise_divide axpy axpy
        copy copy axpy axpy copy fill copy copy
        fill stiffness_apply_planned mass_apply mass_apply pointwise_divide axpy axpy copy
        copy axpy axpy copy fill copy copy fill
        stiffness_apply_planned mass_apply mass_apply pointwise_divide axpy axpy probe_eval element_receive
        field_accumulate
    """.split(),
    "linear-reference-sequence-array": """
        copy copy copy copy axpy axpy copy copy
        copy fill stiffness_apply_planned facet_source_array mass_apply pointwise_divide axpy axpy
        copy copy axpy axpy copy copy copy fill
        stiffness_apply_planned facet_source_array mass_apply pointwise_divide axpy axpy copy copy
        axpy axpy copy copy copy fill stiffness_apply_planned facet_source_array
        mass_apply pointwise_divide axpy axpy copy copy axpy axpy
        copy copy copy fill stiffness_apply_planned facet_source_array mass_apply pointwise_divide
        axpy axpy probe_eval element_receive field_accumulate
    """.split(),
    "linear-reference-sequence-sponge-points-relaxation": """
        copy copy copy copy axpy axpy copy fill
        copy copy fill stiffness_apply_planned mass_apply mass_apply sponge_terms point_source
        pointwise_divide axpy axpy relax_stage copy copy axpy axpy
        copy fill copy copy fill stiffness_apply_planned mass_apply mass_apply
        sponge_terms point_source pointwise_divide axpy axpy relax_stage copy copy
        axpy axpy copy fill copy copy fill stiffness_apply_planned
        mass_apply mass_apply sponge_terms point_source pointwise_divide axpy axpy relax_stage
        copy copy axpy axpy copy fill copy copy
        fill stiffness_apply_planned mass_apply mass_apply sponge_terms point_source pointwise_divide axpy
        axpy relax_stage probe_eval element_receive field_accumulate
    """.split(),
    "westervelt-fused-plain": """
        fill fill copy copy westervelt_cell_apply_planned facet_terms rk4_stage_nl2 westervelt_cell_apply_planned
        facet_terms rk4_stage_nl2 westervelt_cell_apply_planned facet_terms rk4_stage_nl2 westervelt_cell_apply_planned facet_terms rk4_stage_nl2
        probe_eval element_receive field_accumulate copy copy
    """.split(),
    "westervelt-fused-array": """
        fill fill copy copy westervelt_cell_apply_planned facet_source_array rk4_stage_nl2 westervelt_cell_apply_planned
        facet_source_array rk4_stage_nl2 westervelt_cell_apply_planned facet_source_array rk4_stage_nl2 westervelt_cell_apply_planned facet_source_array rk4_stage_nl2
        probe_eval element_receive field_accumulate copy copy
    """.split(),
    "westervelt-fused-sponge-points-relaxation": """
        fill fill copy copy westervelt_cell_apply_planned facet_terms sponge_terms point_source
        relax_stage rk4_stage_nl2 westervelt_cell_apply_planned facet_terms sponge_terms point_source relax_stage rk4_stage_nl2
        westervelt_cell_apply_planned facet_terms sponge_terms point_source relax_stage rk4_stage_nl2 westervelt_cell_apply_planned facet_terms
        sponge_terms point_source rk4_stage_nl2 relax_stage probe_eval element_receive field_accumulate copy
        copy
    """.split(),
    "westervelt-reference-sequence-plain": """
        copy copy copy copy axpy axpy copy fill
        fill copy copy square fill mass_apply axpy fill
        stiffness_apply_planned stiffness_apply_planned mass_apply mass_apply mass_apply mass_apply pointwise_divide axpy
        axpy copy copy axpy axpy copy fill fill
        copy copy square fill mass_apply axpy fill stiffness_apply_planned
        stiffness_apply_planned mass_apply mass_apply mass_apply mass_apply pointwise_divide axpy axpy
        copy copy axpy axpy copy fill fill copy
        copy square fill mass_apply axpy fill stiffness_apply_planned stiffness_apply_planned
        mass_apply mass_apply mass_apply mass_apply pointwise_divide axpy axpy copy
        copy axpy axpy copy fill fill copy copy
        square fill mass_apply axpy fill stiffness_apply_planned stiffness_apply_planned mass_apply
        mass_apply mass_apply mass_apply pointwise_divide axpy axpy probe_eval element_receive
        field_accumulate
    """.split(),
    "westervelt-reference-sequence-array": """
        copy copy copy copy axpy axpy copy copy
        copy square fill mass_apply axpy fill stiffness_apply_planned stiffness_apply_planned
        mass_apply facet_source_array mass_apply pointwise_divide axpy axpy copy copy
        axpy axpy copy copy copy square fill mass_apply
        axpy fill stiffness_apply_planned stiffness_apply_planned mass_apply facet_source_array mass_apply pointwise_divide
        axpy axpy copy copy axpy axpy copy copy
        copy square fill mass_apply axpy fill stiffness_apply_planned stiffness_apply_planned
        mass_apply facet_source_array mass_apply pointwise_divide axpy axpy copy copy
        axpy axpy copy copy copy square fill mass_apply
        axpy fill stiffness_apply_planned stiffness_apply_planned mass_apply facet_source_array mass_apply pointwise_divide
        axpy axpy probe_eval element_receive field_accumulate
    """.split(),
    "westervelt-reference-sequence-sponge-points-relaxation": """
        copy copy copy copy axpy axpy copy fill
        fill copy copy square fill mass_apply axpy fill
        stiffness_apply_planned stiffness_apply_planned mass_apply mass_apply mass_apply mass_apply sponge_terms point_source
        pointwise_divide axpy axpy relax_stage copy copy axpy axpy
        copy fill fill copy copy square fill mass_apply
        axpy fill stiffness_apply_planned stiffness_apply_planned mass_apply mass_apply mass_apply mass_apply
        sponge_terms point_source pointwise_divide axpy axpy relax_stage copy copy
        axpy axpy copy fill fill copy copy square
        fill mass_apply axpy fill stiffness_apply_planned stiffness_apply_planned mass_apply mass_apply
        mass_apply mass_apply sponge_terms point_source pointwise_divide axpy axpy relax_stage
        copy copy axpy axpy copy fill fill copy
        copy square fill mass_apply axpy fill stiffness_apply_planned stiffness_apply_planned
        mass_apply mass_apply mass_apply mass_apply sponge_terms point_source pointwise_divide axpy
        axpy relax_stage probe_eval element_receive field_accumulate
    """.split(),
}


@pytest.mark.parametrize("extras", ["plain", "array", "sponge-points-relaxation"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "reference-sequence"])
@pytest.mark.parametrize("which", ["linear", "westervelt"])
def test_one_step_calls_the_pinned_entries(library, which, fused, extras):
    import torch

    mesh, dt = _mesh()
    s = _solver(which, mesh, fused, extras)
    rec = _recorders(mesh, s)
    s.init()
    s.rk4(0.0, 100 * dt, dt, max_steps=1)
    torch.cuda.synchronize()
    library.on = True
    t, steps = s.rk4(dt, 100 * dt, dt, max_steps=1, **rec)
    library.on = False
    torch.cuda.synchronize()
    assert steps == 1 and rec["sensors"].nrec == rec["receivers"].nrec == rec["monitor"].nacc == 1
    assert np.max(np.abs(s.u_sol())) > 0
    key = f"{which}-{'fused' if fused else 'reference-sequence'}-{extras}"
    got = _words(library.names)
    print(f"{key}:\n    " + "\n    ".join(" ".join(got[i:i + 8]) for i in range(0, len(got), 8)))
    assert got == EXPECTED[key]


@pytest.mark.parametrize("extras", ["plain", "array"])
def test_graph_replay_equals_rk4(library, extras):
    """``rk4_graph`` over three steps against ``rk4`` on a second solver, at the bar of the graph-replay tests of
    tests/test_solver_gpu.py (1e-13).  Not bitwise: on this mesh a dof of b receives the float-atomic adds of up to eight cells, and on
    the commit the lists were recorded from two ``rk4`` runs already differed in the last bits (6 of 6 trials, by 1e-19 to 3e-16, as
    ``rk4_graph`` from ``rk4``)."""
    mesh, dt = _mesh()
    a, b = (_solver("linear", mesh, True, extras) for _ in range(2))
    a.init(), b.init()
    assert a.rk4(0.0, 100 * dt, dt, max_steps=3)[1] == 3
    assert b.rk4_graph(0.0, 100 * dt, dt, max_steps=3)[1] == 3 and len(b._graphs) == 1
    assert np.max(np.abs(a.u_sol())) > 0
    du, dv = rel_l2(b.u_sol(), a.u_sol()), rel_l2(b.v_sol(), a.v_sol())
    print(f"{extras}: rk4_graph against rk4, rel l2 u {du:.3e} v {dv:.3e}")
    assert du < 1e-13 and dv < 1e-13
