"""Which C entry points ``operators.py`` calls, in which order, pinned on the CPU with a recording stand-in for the library (no GPU):
the route of a mass apply and the name ``mass_kernel_name`` reports for it, the forms of the stiffness, gradient and Westervelt cell
operators, the facet terms with empty sets, and the three workspace caches (capacity, clear, hold list, identity key)."""

import ctypes as C
import types

import numpy as np
import pytest
import torch

from conftest import pkg

EPB = 8  # the stand-in's entities per batch
SWITCHES = ("_USE_PLAN", "_LOCALITY_ORDER", "_STRIP_ORDER", "_USE_GATHER", "_MASS_PLAN_MIN_ENTRIES", "_GATHER_MAX_MEAN_ENTRIES",
            "_GATHER_STATIC_MAX_MEAN_ENTRIES")


class _Library:
    """Every ``fus_*`` attribute is a function that records (name, arguments) and returns 0.  An argument is recorded by the type
    ``_lib.SIGNATURES`` declares for it: "null" / "ptr" for a pointer, the value for a number."""

    def __init__(self, signatures):
        self.signatures, self.calls, self.raw = signatures, [], []
        self.touched = 0  # what fus_mass_gather_plan_info reports as info[0]
        self.refuse = set()  # entry names answered with ERR_UNSUPPORTED_ENTITY

    def __getattr__(self, name):
        if not name.startswith("fus_"):
            raise AttributeError(name)
        sig = self.signatures[name]  # KeyError: an entry the ABI does not declare

        def fn(*args):
            assert len(args) == len(sig), f"{name}: {len(args)} arguments, the ABI declares {len(sig)}"
            seen = []
            for a, t in zip(args, sig):
                if t is C.c_void_p:
                    null = a is None or (isinstance(a, C.c_void_p) and not a.value)
                    seen.append("null" if null else "ptr")
                else:
                    seen.append(a)
            self.calls.append((name, tuple(seen)))
            self.raw.append((name, args))
            if name in self.refuse:
                return -3  # _lib.ERR_UNSUPPORTED_ENTITY
            if name == "fus_plan_entities_per_batch":
                return EPB
            if name.endswith("_bytes"):
                return 64
            if name == "fus_mass_gather_plan_info":
                args[1][0] = self.touched
            return 0

        return fn

    def take(self):
        """-> the entry names called since the last ``take``."""
        names = [c[0] for c in self.calls]
        self.last = list(self.calls)
        self.calls.clear()
        return names

    def released(self):
        return [args[0] for name, args in self.raw if name == "fus_plan_release"]


def _req_host(t, dtype, name):
    """``_lib.require_device_tensor`` without the ``is_cuda`` check."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a device array, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: array must be C-contiguous")
    return t


class _TorchOnHost:
    """``torch`` as the module under test sees it: the current device is the CPU."""

    cuda = types.SimpleNamespace(current_device=lambda: 0)

    @staticmethod
    def device(*_):
        return torch.device("cpu")

    def __getattr__(self, name):
        return getattr(torch, name)


@pytest.fixture
def rt(monkeypatch):
    ops, lib_mod = pkg("operators"), pkg("_lib")
    lib = _Library(lib_mod.SIGNATURES)
    monkeypatch.setattr(lib_mod, "load", lambda: lib)
    monkeypatch.setattr(lib_mod, "stream_ptr", lambda: C.c_void_p(None))
    monkeypatch.setattr(lib_mod, "require_device_tensor", _req_host)
    monkeypatch.setattr(ops, "_req", _req_host)
    monkeypatch.setattr(ops, "torch", _TorchOnHost())
    for name in SWITCHES:  # restored after the test, whatever it assigns
        monkeypatch.setattr(ops, name, getattr(ops, name))
    ops.use_plan(True)
    ops.use_mass_gather(True)
    ops.use_locality_order(False)
    ops.use_strip_order(False)
    ops._MASS_PLAN_MIN_ENTRIES, ops._GATHER_MAX_MEAN_ENTRIES, ops._GATHER_STATIC_MAX_MEAN_ENTRIES = 1 << 15, 2.6, 4.0
    ops._PLANS.clear()
    lib.calls.clear()
    lib.raw.clear()
    yield types.SimpleNamespace(ops=ops, lib=lib, lib_mod=lib_mod)
    ops._PLANS.clear()  # nothing of the stand-in's stays in the module's caches


def _mass_args(N, nent, ndofs, dtype=torch.float64):
    x, y = torch.zeros(ndofs, dtype=dtype), torch.zeros(ndofs, dtype=dtype)
    return x, torch.ones(nent, dtype=dtype), y, torch.ones((nent, N), dtype=dtype), torch.zeros((nent, N), dtype=torch.int32)


GATHER_SETUP = ["fus_mass_gather_plan_bytes", "fus_mass_gather_plan_build", "fus_mass_gather_plan_info"]
PLAN_SETUP = ["fus_plan_entities_per_batch", "fus_plan_bytes", "fus_plan_build_ordered"]
STATIC_SETUP = ["fus_mass_gather_static_bytes", "fus_mass_gather_static_build_f64"]

# (N, entities, touched dofs, operator keywords) -> set-up entries of the first call, the apply, mass_kernel_name
MASS_TABLE = {
    "gather-2.0": ((125, 300, 18750, {}), GATHER_SETUP, "fus_mass_apply_gather_f64", "fus::mass_gather_kernel"),
    "static-only-3.0": ((27, 2000, 18000, {}), GATHER_SETUP + PLAN_SETUP, "fus_mass_apply_planned_f64", "fus::mass_plan_kernel"),
    "static-3.0": ((27, 2000, 18000, {"static_detJ": True}), GATHER_SETUP + STATIC_SETUP, "fus_mass_apply_gather_static_f64",
                   "fus::mass_gather_kernel"),
    "dense-8.0": ((8, 5000, 5000, {}), GATHER_SETUP + ["fus_plan_release"] + PLAN_SETUP, "fus_mass_apply_planned_f64",
                  "fus::mass_plan_kernel"),
    "atomic": ((125, 300, 18750, {"atomic": True}), PLAN_SETUP, "fus_mass_apply_planned_f64", "fus::mass_plan_kernel"),
    "small": ((125, 10, 1000, {}), [], "fus_mass_apply_f64", "fus::mass_kernel"),
}


@pytest.mark.parametrize("case", list(MASS_TABLE))
def test_mass_route_table(rt, case):
    (N, nent, touched, kw), setup, apply, kernel = MASS_TABLE[case]
    rt.lib.touched = touched
    args = _mass_args(N, nent, touched)
    op = rt.ops.mass_operator(N, np.float64, **kw)
    op(*args)
    assert rt.lib.take() == setup + [apply]
    op(*args)
    assert rt.lib.take() == [apply]  # the second call is the apply alone
    name = rt.ops.mass_kernel_name(args[4], touched, atomic=kw.get("atomic", False), static=kw.get("static_detJ", False))
    assert name == kernel
    assert rt.lib.take() == []  # every plan it asks for is cached by now
    # the apply's arguments: five pointers, then the integers, then the (null) stream
    op(*args)
    ints = (N, EPB, nent) if apply == "fus_mass_apply_planned_f64" else (N, nent)
    assert rt.lib.calls == [(apply, ("ptr",) * 5 + ints + ("null",))]


def test_mass_kernel_name_builds_only_the_gather_plan(rt):
    """Asked before any apply, it builds the transposed plan it judges by and nothing else."""
    rt.lib.touched = 18000
    dm = _mass_args(27, 2000, 18000)[4]
    assert rt.ops.mass_kernel_name(dm, 18000) == "fus::mass_plan_kernel"
    assert rt.lib.take() == GATHER_SETUP
    assert rt.ops.mass_kernel_name(dm, 18000, static=True) == "fus::mass_gather_kernel"
    assert rt.ops.mass_kernel_name(dm, 18000, atomic=True, static=True) == "fus::mass_plan_kernel"
    assert rt.lib.take() == []


def test_mass_launch_form_and_dtype(rt):
    rt.lib.touched = 18750
    args = _mass_args(125, 300, 18750, torch.float32)
    rt.ops.mass_operator[1, 1](*args)  # the cuda flavour: no N, no dtype fixed
    assert rt.lib.take() == GATHER_SETUP + ["fus_mass_apply_gather_f32"]
    with pytest.raises(TypeError):
        rt.ops.mass_operator(125, np.float64)(*args)
    assert rt.lib.take() == []


def test_mass_switches(rt):
    rt.lib.touched = 18750
    args = _mass_args(125, 300, 18750)
    op = rt.ops.mass_operator(125, np.float64)
    rt.ops.use_mass_gather(False)
    op(*args)
    assert rt.lib.take() == PLAN_SETUP + ["fus_mass_apply_planned_f64"]
    assert rt.ops.mass_kernel_name(args[4], 18750) == "fus::mass_plan_kernel"
    rt.ops.use_plan(False)
    op(*args)
    assert rt.lib.take() == ["fus_mass_apply_f64"]
    assert rt.ops.mass_kernel_name(args[4], 18750) == "fus::mass_kernel"
    rt.ops.use_mass_gather(True)  # the gather does not depend on the batch-plan switch
    op(*args)
    assert rt.lib.take() == GATHER_SETUP + ["fus_mass_apply_gather_f64"]
    assert rt.ops.mass_kernel_name(args[4], 18750) == "fus::mass_gather_kernel"


def test_mass_plan_min_entries_assigned_on_the_module(rt):
    rt.lib.touched = 1000
    args = _mass_args(125, 10, 1000)
    op = rt.ops.mass_operator(125, np.float64)
    op(*args)
    assert rt.lib.take() == ["fus_mass_apply_f64"]
    rt.ops._MASS_PLAN_MIN_ENTRIES = 1
    op(*args)
    assert rt.lib.take() == GATHER_SETUP + ["fus_mass_apply_gather_f64"]
    assert rt.ops.mass_kernel_name(args[4], 1000) == "fus::mass_gather_kernel"
    one = _mass_args(1, 40, 40)  # one dof per entity: no batch plan (its batches hold 2 .. 4096 dofs per entity)
    rt.ops.mass_operator(1, np.float64, atomic=True)(*one)
    assert rt.lib.take() == ["fus_mass_apply_f64"]
    assert rt.ops.mass_kernel_name(one[4], 40, atomic=True) == "fus::mass_kernel"


def test_gather_build_refused_takes_the_batch_plan(rt):
    rt.lib.refuse.add("fus_mass_gather_plan_build")
    args = _mass_args(125, 300, 18750)
    op = rt.ops.mass_operator(125, np.float64)
    op(*args)
    assert rt.lib.take() == GATHER_SETUP[:2] + PLAN_SETUP + ["fus_mass_apply_planned_f64"]
    assert rt.ops._GATHER_PLANS.get(args[4], 18750) is None  # ... and the refusal is cached
    op(*args)
    assert rt.lib.take() == ["fus_mass_apply_planned_f64"]
    assert rt.ops.mass_kernel_name(args[4], 18750) == "fus::mass_plan_kernel"


def test_gather_build_error_raises(rt, monkeypatch):
    """Any other answer of the build is an error, not a refusal."""
    monkeypatch.setattr(rt.lib_mod, "check", lambda rc, what="": (_ for _ in ()).throw(rt.lib_mod.FusGpuError(what)) if rc else None)
    monkeypatch.setattr(_Library, "fus_mass_gather_plan_build", lambda self, *a: -1, raising=False)
    with pytest.raises(rt.lib_mod.FusGpuError):
        rt.ops.mass_operator(125, np.float64)(*_mass_args(125, 300, 18750))


@pytest.mark.parametrize("static_only", [True, False], ids=["static-only-plan", "plain-plan"])
def test_static_build_refused_takes_the_default_path(rt, static_only):
    """No static companion: the apply the default operator would launch, and ``None`` cached for the companion."""
    N, nent, touched = (27, 2000, 18000) if static_only else (125, 300, 18750)
    rt.lib.touched = touched
    rt.lib.refuse.add("fus_mass_gather_static_build_f64")
    args = _mass_args(N, nent, touched)
    op = rt.ops.mass_operator(N, np.float64, static_detJ=True)
    op(*args)
    default = PLAN_SETUP + ["fus_mass_apply_planned_f64"] if static_only else ["fus_mass_apply_gather_f64"]
    assert rt.lib.take() == GATHER_SETUP + STATIC_SETUP + default
    assert list(rt.ops._STATIC_DETJ._entries.values()) == [None]
    op(*args)
    assert rt.lib.take() == default[-1:]


def test_static_build_refused_checks_once(rt, monkeypatch):
    """... with every argument checked once and each cache asked once."""
    rt.lib.touched = 18000
    rt.lib.refuse.add("fus_mass_gather_static_build_f64")
    args = _mass_args(27, 2000, 18000)
    op = rt.ops.mass_operator(27, np.float64, static_detJ=True)
    checked, asked = [], []
    gather_get, static_get = rt.ops._GATHER_PLANS.get, rt.ops._STATIC_DETJ.get
    monkeypatch.setattr(rt.ops, "_req", lambda t, dt, name: (checked.append(name), _req_host(t, dt, name))[1])
    monkeypatch.setattr(rt.ops._GATHER_PLANS, "get", lambda *a, **k: (asked.append("gather"), gather_get(*a, **k))[1])
    monkeypatch.setattr(rt.ops._STATIC_DETJ, "get", lambda *a, **k: (asked.append("static"), static_get(*a, **k))[1])
    op(*args)
    assert rt.lib.take()[-1] == "fus_mass_apply_planned_f64"
    assert sorted(checked) == sorted(["x", "entity_constants", "y", "entity_detJ", "entity_dofmap"])
    assert asked == ["gather", "static"]


def test_static_refresh_forgets_the_companions(rt):
    rt.lib.touched = 18000
    args = _mass_args(27, 2000, 18000)
    op = rt.ops.mass_operator(27, np.float64, static_detJ=True)
    op(*args)
    (entry,) = rt.ops._STATIC_DETJ._entries.values()
    rt.lib.take()
    op.refresh()
    assert rt.lib.take() == ["fus_plan_release"] and rt.lib.released()[-1] == entry[0].data_ptr()
    op(*args)
    assert rt.lib.take() == STATIC_SETUP + ["fus_mass_apply_gather_static_f64"]
    assert op.atomic is not op and op.atomic.atomic is op.atomic
    op.atomic(*args)  # the atomic twin of a static operator is a plain atomic one
    assert rt.lib.take() == PLAN_SETUP + ["fus_mass_apply_planned_f64"]


def test_mass_exclusive_marks(rt):
    args = _mass_args(125, 300, 18750)
    rt.ops.mass_operator(125, np.float64, exclusive=True, atomic=True)(*args)
    assert rt.lib.take() == PLAN_SETUP + ["fus_plan_mark_exclusive", "fus_mass_apply_planned_f64"]
    (key,) = rt.ops._PLANS._plans
    assert key[5] == (18750, None)


def test_apply_rows_and_rows_available(rt):
    rt.lib.touched = 18750
    x, c, y, detJ, dm = args = _mass_args(125, 300, 18750)
    rows = torch.zeros(18750, dtype=torch.uint8)
    op = rt.ops.mass_operator(125, np.float64)
    ROWS_SETUP = ["fus_mass_gather_plan_bytes", "fus_mass_gather_plan_build_rows", "fus_mass_gather_plan_info"]
    assert op.rows_available(dm, 18750, rows) and not op.atomic.rows_available(dm, 18750, rows)
    assert rt.lib.take() == GATHER_SETUP + ROWS_SETUP + ROWS_SETUP
    assert [c_[1][5] for c_ in rt.lib.last if c_[0].endswith("_rows")] == [0, 1]  # which half
    op.apply_rows(*args, rows, 1)
    assert rt.lib.take() == ["fus_mass_apply_gather_f64"]
    assert rt.ops.mass_rows_available(dm, 18750, rows)
    assert rt.lib.take() == []
    with pytest.raises(ValueError):
        rt.ops._GATHER_PLANS.get(dm, 18750, (rows[:-1], 0))
    with pytest.raises(TypeError):
        op.apply_rows(x.float(), c, y, detJ, dm, rows, 1)
    with pytest.raises(ValueError):
        op.apply_rows(x, c[:-1], y, detJ, dm, rows, 1)
    assert rt.lib.take() == []


def test_apply_rows_without_a_plan(rt):
    rt.lib.touched = 18750
    rt.lib.refuse.add("fus_mass_gather_plan_build_rows")
    args = _mass_args(125, 300, 18750)
    rows = torch.zeros(18750, dtype=torch.uint8)
    op = rt.ops.mass_operator(125, np.float64)
    assert not op.rows_available(args[4], 18750, rows)
    with pytest.raises(rt.lib_mod.FusGpuError, match="row-subset"):
        op.apply_rows(*args, rows, 0)
    assert "fus_mass_apply_gather_f64" not in rt.lib.take()
    # a dofmap the gather is not used for has no rows either, and nothing is built to find that out
    small = _mass_args(125, 10, 1000)
    assert not op.rows_available(small[4], 1000, torch.zeros(1000, dtype=torch.uint8))
    rt.ops.use_mass_gather(False)
    assert not op.rows_available(args[4], 18750, rows)
    assert rt.lib.take() == []


def test_mass_argument_errors(rt):
    x, c, y, detJ, dm = _mass_args(125, 300, 18750)
    for static in (False, True):
        op = rt.ops.mass_operator(125, np.float64, static_detJ=static)
        with pytest.raises(TypeError):
            op(x.float(), c, y, detJ, dm)
        with pytest.raises(TypeError):
            op(x, c, y, detJ, dm.long())
        with pytest.raises(TypeError):
            op(x.numpy(), c, y, detJ, dm)
        with pytest.raises(ValueError):
            op(x, c, y, detJ[:, :-1].contiguous(), dm)
        with pytest.raises(ValueError):
            op(x, c[:-1], y, detJ, dm)
        with pytest.raises(ValueError):
            rt.ops.mass_operator(27, np.float64, static_detJ=static)(x, c, y, detJ, dm)
        op(x, c[:0], y, detJ[:0], dm[:0])  # no entities: nothing to do
    assert rt.lib.take() == []


# ------------------------------------------------------------------------------------------------------------- cell operators
def _cell_args(P, ncell, ndofs=50, dtype=torch.float64):
    nd = (P + 1) ** 3
    z = lambda *s: torch.zeros(s, dtype=dtype)  # noqa: E731
    return types.SimpleNamespace(x=z(ndofs), y=z(ndofs), cc=z(ncell), G=z(ncell, nd, 6), detJ=z(ncell, nd),
                                 dm=torch.zeros((ncell, nd), dtype=torch.int32), x_dofs=torch.zeros((ncell, 8), dtype=torch.int32),
                                 x_g=np.zeros((2 * ncell, 3)), pts=np.zeros(P + 1), wts=np.ones(P + 1), D=np.zeros((P + 1) ** 2))


def _plan_keys(ops):
    return [k[-1] == "strips" for k in ops._PLANS._plans]


@pytest.mark.parametrize("strip_order", [False, True])
def test_stiffness_forms(rt, strip_order):
    ops, P, ncell = rt.ops, 2, 5
    a = _cell_args(P, ncell)
    ops.use_strip_order(strip_order)
    forms = {
        "fus_stiffness_apply_planned_geom_f64": ops.stiffness_operator(P, a.D, np.float64, geometry=(a.x_dofs, a.x_g, a.pts, a.wts)),
        "fus_stiffness_apply_planned_affine_f64": ops.stiffness_operator(P, a.D, np.float64, affine_weights=np.ones(27)),
        "fus_stiffness_apply_planned_f64": ops.stiffness_operator(P, a.D, np.float64),
    }
    assert rt.lib.take() == []  # no library call at construction
    for entry, op in forms.items():
        ops._PLANS.clear()
        rt.lib.take()
        op(a.x, a.cc, a.y, None if "geom" in entry else a.G, a.dm)
        assert rt.lib.take() == PLAN_SETUP + [entry]
        assert rt.lib.last[-1][1][-3:] == (P, ncell, "null") and "null" not in rt.lib.last[-1][1][:-1]
        # the geometry and affine forms key their plan apart only under use_strip_order(True)
        assert _plan_keys(ops) == [strip_order and entry != "fus_stiffness_apply_planned_f64"]
        op(a.x, a.cc, a.y, a.x_dofs if "geom" in entry else a.G, a.dm)  # (geometry form: x_dofs rows in the G position)
        assert rt.lib.take() == [entry]
        ops._PLANS.clear()
        rt.lib.take()
        op.prepare(a.dm)
        assert rt.lib.take() == PLAN_SETUP and _plan_keys(ops) == [strip_order and entry != "fus_stiffness_apply_planned_f64"]
    ops.use_plan(False)
    ops._PLANS.clear()
    rt.lib.take()
    forms["fus_stiffness_apply_planned_f64"](a.x, a.cc, a.y, a.G, a.dm)
    assert rt.lib.take() == ["fus_stiffness_apply_f64"] and not ops._PLANS._plans
    forms["fus_stiffness_apply_planned_f64"].prepare(a.dm)
    assert rt.lib.take() == []


def test_stiffness_cuda_flavour_and_errors(rt):
    ops, P, ncell = rt.ops, 2, 5
    a = _cell_args(P, ncell, dtype=torch.float32)
    op = ops.stiffness_operator(P, np.float32)
    with pytest.raises(TypeError):
        op(a.x, a.cc, a.y, a.G, a.dm)  # built without a table
    op[4, 64](a.x, a.cc, a.y, a.G, a.dm, a.D.reshape(3, 3))
    assert rt.lib.take() == PLAN_SETUP + ["fus_stiffness_apply_planned_f32"]
    with pytest.raises(ValueError):
        op[4, 64](a.x, a.cc, a.y, a.G, a.dm, np.zeros(8))
    with pytest.raises(TypeError):
        op[4, 64](a.x.double(), a.cc, a.y, a.G, a.dm, a.D)
    with pytest.raises(TypeError):
        op[4, 64](a.x, a.cc, a.y, a.G, a.dm.long(), a.D)
    with pytest.raises(ValueError):
        op[4, 64](a.x, a.cc, a.y, a.G[:, :5].contiguous(), a.dm, a.D)
    with pytest.raises(ValueError):
        op[4, 64](a.x, a.cc[:-1], a.y, a.G, a.dm, a.D)
    op[4, 64](a.x, a.cc[:0], a.y, a.G[:0], a.dm[:0], a.D)  # no cells: nothing to do
    for bad in (0, 11):
        with pytest.raises(ValueError):
            ops.stiffness_operator(bad, np.float64)
    with pytest.raises(ValueError):
        ops.stiffness_operator(P, a.D, np.float64, affine_weights=np.ones(26))
    with pytest.raises(ValueError):
        ops.stiffness_operator(P, a.D, np.float64, geometry=(a.x_dofs, a.x_g, a.pts[:-1], a.wts))
    with pytest.raises(ValueError):
        ops.stiffness_operator(P, a.D, np.float64, geometry=(a.x_dofs[:, :7], a.x_g, a.pts, a.wts))
    with pytest.raises(TypeError):
        ops.stiffness_operator(P)
    geom = ops.stiffness_operator(P, a.D, np.float32, geometry=(a.x_dofs[:-1], a.x_g, a.pts, a.wts))
    with pytest.raises(ValueError, match="x_dofs"):
        geom(a.x, a.cc, a.y, None, a.dm)
    assert rt.lib.take() == []


def test_gradient_operator(rt):
    ops, P, ncell = rt.ops, 2, 5
    a = _cell_args(P, ncell)
    op = ops.gradient_operator(P, a.D, np.float64, geometry=(a.x_dofs, a.x_g, a.pts, a.wts))
    assert (op.P, op.n, op.dtype) == (2, 3, torch.float64) and rt.lib.take() == []
    y3 = torch.zeros((3, 64), dtype=torch.float64)[:, :50]  # rows further apart than ndofs
    op(a.x, a.cc, y3, a.dm)
    assert rt.lib.take() == PLAN_SETUP + ["fus_gradient_apply_planned_geom_f64"]
    seen = rt.lib.last[-1][1]
    assert seen[3] == 64 and seen[-3:] == (P, ncell, "null") and "null" not in seen[:-1]
    ops._PLANS.clear()
    rt.lib.take()
    op.prepare(a.dm)
    assert rt.lib.take() == PLAN_SETUP
    ops.use_strip_order(True)
    op(a.x, a.cc, y3, a.dm)
    assert rt.lib.take() == PLAN_SETUP + ["fus_gradient_apply_planned_geom_f64"] and _plan_keys(ops) == [False, True]
    with pytest.raises(TypeError):
        op(a.x, a.cc, y3.float(), a.dm)
    with pytest.raises(ValueError):
        op(a.x, a.cc, y3[:, :-1], a.dm)
    with pytest.raises(ValueError):
        op(a.x, a.cc, y3.T.contiguous(), a.dm)
    with pytest.raises(ValueError):
        op(a.x, a.cc[:-1], y3, a.dm)
    short = ops.gradient_operator(P, a.D, np.float64, geometry=(a.x_dofs[:-1], a.x_g, a.pts, a.wts))
    with pytest.raises(ValueError, match="x_dofs"):
        short(a.x, a.cc, y3, a.dm)
    for bad in (None, (a.x_dofs, a.x_g, a.pts)):
        with pytest.raises(ValueError):
            ops.gradient_operator(P, a.D, np.float64, geometry=bad)
    with pytest.raises(ValueError):
        ops.gradient_operator(P, None, np.float64, geometry=(a.x_dofs, a.x_g, a.pts, a.wts))
    assert rt.lib.take() == []


@pytest.mark.parametrize("geom", [False, True], ids=["tables", "in-kernel-geometry"])
def test_westervelt_forms(rt, geom):
    ops, P, ncell = rt.ops, 2, 5
    a = _cell_args(P, ncell)
    ops.use_strip_order(True)
    op = ops.westervelt_cell_operator(P, a.D, np.float64, geometry=(a.x_g, a.pts, a.wts) if geom else None)
    assert (op.P, op.n, op.dtype) == (2, 3, torch.float64) and rt.lib.take() == []
    entry = "fus_westervelt_cell_apply_planned_geom_f64" if geom else "fus_westervelt_cell_apply_planned_f64"
    tail = (a.x_dofs, a.dm) if geom else (a.G, a.detJ, a.dm)
    op(a.x, a.x, a.cc, a.cc, a.cc, a.cc, a.y, a.y, *tail)
    assert rt.lib.take() == PLAN_SETUP + [entry]
    full = rt.lib.last[-1][1]
    assert "null" not in full[:-1] and full[-3:] == (P, ncell, "null")
    assert _plan_keys(ops) == [geom]  # the in-kernel-geometry form keys its plan with "strips"
    op.stiffness_only(a.x, a.x, a.cc, a.cc, a.y, *((a.x_dofs, a.dm) if geom else (a.G, a.dm)))
    assert rt.lib.take() == [entry]  # the same entry as the full call ...
    part = rt.lib.last[-1][1]
    null = [i for i, v in enumerate(part[:-1]) if v == "null"]
    assert null == ([2, 5, 7] if geom else [2, 5, 7, 9])  # ... without c2, c5, m (and detJ)
    assert len(part) == len(full) and part[-3:] == full[-3:]
    with pytest.raises(TypeError):
        op(a.x.float(), a.x, a.cc, a.cc, a.cc, a.cc, a.y, a.y, *tail)
    with pytest.raises(ValueError):
        op(a.x, a.x, a.cc, a.cc, a.cc[:-1], a.cc, a.y, a.y, *tail)
    with pytest.raises(ValueError):
        op(a.x, a.x, a.cc, a.cc, a.cc, a.cc, a.y, a.y, *((a.x_dofs[:-1], a.dm) if geom else (a.G[:-1], a.detJ, a.dm)))
    with pytest.raises(ValueError):
        op.stiffness_only(a.x, a.x, a.cc, a.cc[:-1], a.y, *((a.x_dofs, a.dm) if geom else (a.G, a.dm)))
    with pytest.raises(ValueError):
        op.stiffness_only(a.x, a.x, a.cc, a.cc, a.y, *((a.x_dofs[:-1], a.dm) if geom else (a.G[:-1], a.dm)))
    with pytest.raises(TypeError):
        op.stiffness_only(a.x, a.x, a.cc, a.cc, a.y, *((a.x_dofs.long(), a.dm) if geom else (a.G.float(), a.dm)))
    e = _cell_args(P, 0)
    op(e.x, e.x, e.cc, e.cc, e.cc, e.cc, e.y, e.y, *((e.x_dofs, e.dm) if geom else (e.G, e.detJ, e.dm)))
    op.stiffness_only(e.x, e.x, e.cc, e.cc, e.y, *((e.x_dofs, e.dm) if geom else (e.G, e.dm)))
    assert rt.lib.take() == []
    with pytest.raises(ValueError):
        ops.westervelt_cell_operator(11, a.D, np.float64)
    if geom:
        with pytest.raises(ValueError):
            ops.westervelt_cell_operator(P, a.D, np.float64, geometry=(a.x_g, a.pts[:-1], a.wts))


# --------------------------------------------------------------------------------------------------------------- facet terms
def _facets(nA, nB, N=9, ndofs=40, dtype=torch.float64):
    z = lambda *s: torch.zeros(s, dtype=dtype)  # noqa: E731
    dmA, dmB = torch.zeros((nA, N), dtype=torch.int32), torch.zeros((nB, N), dtype=torch.int32)
    return z(ndofs), (z(nA), 0.5, z(nA), 0.25, z(nA, N), dmA), (z(ndofs), z(nB), z(nB, N), dmB)


def _bound_array(nA, N=9, dtype=torch.float64, coeff2=True):
    z = lambda *s: torch.zeros(s, dtype=dtype)  # noqa: E731
    return types.SimpleNamespace(dtype=dtype, nfacets=nA, coeff1=z(nA), coeff2=z(nA) if coeff2 else None, detJ=z(nA, N),
                                 dofmap=torch.zeros((nA, N), dtype=torch.int32), element_of_facet=torch.zeros(nA, dtype=torch.int32),
                                 amplitude=torch.zeros(3, dtype=torch.float64), phase=torch.zeros(3, dtype=torch.float64),
                                 delay=torch.zeros(3, dtype=torch.float64), n_elements=3)


@pytest.mark.parametrize("dev", [False, True], ids=["host-scalars", "device-scalars"])
def test_facet_terms(rt, dev):
    ops = rt.ops
    entry = "fus_facet_terms_dev_f64" if dev else "fus_facet_terms_f64"
    scalars = torch.zeros(2, dtype=torch.float64) if dev else None
    A = ("ptr", "ptr", "ptr") if dev else ("ptr", 0.5, "ptr", 0.25)
    noA = ("null", "null", "ptr") if dev else ("null", 0.5, "null", 0.25)
    for nA, nB in ((4, 6), (0, 6), (4, 0)):
        y, source, field = _facets(nA, nB)
        ops.facet_terms(y, source, field, scalars)
        assert rt.lib.take() == [entry]
        setA = (A if nA else noA) + (("ptr", "ptr") if nA else ("null", "null")) + (nA,)
        setB = (("ptr",) * 4 if nB else ("null",) * 4) + (nB,)
        assert rt.lib.last[-1][1] == ("ptr",) + setA + setB + (9, "null")
    y, source, field = _facets(4, 6)
    ops.facet_terms(y, (source[0], 0.5, None, 0.25) + source[4:], field, scalars)  # no dg term
    assert rt.lib.take() == [entry] and rt.lib.last[-1][1][2 if dev else 3] == "null"
    y, source, field = _facets(0, 0)
    ops.facet_terms(y, source, field, scalars)
    assert rt.lib.take() == []  # both sets empty: no call at all
    y, source, field = _facets(4, 6)
    with pytest.raises(ValueError):
        ops.facet_terms(y, source, field[:2] + (field[2][:, :-1].contiguous(), field[3]), scalars)
    with pytest.raises(ValueError):
        ops.facet_terms(y, source, _facets(4, 6, N=4)[2], scalars)  # another number of dofs per facet
    with pytest.raises(TypeError):
        ops.facet_terms(y.float(), source, field, scalars)
    if dev:
        with pytest.raises(ValueError):
            ops.facet_terms(y, source, field, scalars[:1])
    assert rt.lib.take() == []


@pytest.mark.parametrize("dev", [False, True], ids=["host-stage", "device-stage"])
def test_facet_source_terms(rt, dev):
    ops = rt.ops
    entry = "fus_facet_source_array_dev_f64" if dev else "fus_facet_source_array_f64"
    stage = dict(stage_dev=torch.zeros(6, dtype=torch.float64)) if dev else dict(stage=np.zeros(6))
    for nA, nB, with_field in ((4, 6, True), (0, 6, True), (4, 0, True), (4, 0, False)):
        y, _, field = _facets(nA, nB)
        ops.facet_source_terms(y, _bound_array(nA), field if with_field else None, **stage)
        assert rt.lib.take() == [entry]
        pA, pB = ("ptr" if nA else "null"), ("ptr" if nB else "null")
        assert rt.lib.last[-1][1] == ("ptr",) + (pA,) * 5 + (nA,) + (pA,) * 3 + (3,) + (pB,) * 4 + (nB, 9, "ptr", "null")
    y, _, field = _facets(4, 6)
    ops.facet_source_terms(y, _bound_array(4, coeff2=False), field, **stage)
    assert rt.lib.take() == [entry] and rt.lib.last[-1][1][1:4] == ("ptr", "null", "ptr")
    ops.facet_source_terms(y, _bound_array(0), _facets(0, 0)[2], **stage)
    ops.facet_source_terms(y, _bound_array(0), None, **stage)
    assert rt.lib.take() == []  # both sets empty: no call at all
    with pytest.raises(ValueError):
        ops.facet_source_terms(y, _bound_array(4), field)  # neither stage block
    with pytest.raises(ValueError):
        ops.facet_source_terms(y, _bound_array(4), field, stage=np.zeros(6), stage_dev=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.facet_source_terms(y, _bound_array(4), field, **{k: v[:5] for k, v in stage.items()})
    with pytest.raises(ValueError):
        ops.facet_source_terms(y, _bound_array(4), field[:2] + (field[2][:, :-1].contiguous(), field[3]), **stage)
    with pytest.raises(ValueError):
        ops.facet_source_terms(y, _bound_array(4, N=4), field, **stage)
    with pytest.raises(TypeError):
        ops.facet_source_terms(y, _bound_array(4, dtype=torch.float32), field, **stage)
    assert rt.lib.take() == []


# -------------------------------------------------------------------------------------------------------------------- caches
def _dofmaps(count, nent=3, N=8):
    return [torch.zeros((nent, N), dtype=torch.int32) for _ in range(count)]


def test_plan_cache_drops_and_releases_the_oldest(rt):
    plans = rt.ops._PLANS
    dms = _dofmaps(plans.capacity + 1)
    first = [plans.get(dm)[0] for dm in dms[:-1]]
    assert len(plans._plans) == plans.capacity and rt.lib.released() == []
    plans.get(dms[-1])
    assert len(plans._plans) == plans.capacity and rt.lib.released() == [first[0].data_ptr()]
    assert plans.has(dms[1]) and plans.has(dms[-1]) and not plans.has(dms[0])
    ws, epb = plans.get(dms[1])
    assert ws is first[1] and epb == EPB


def test_gather_and_static_caches_drop_and_release_the_oldest(rt):
    gather, static = rt.ops._GATHER_PLANS, rt.ops._STATIC_DETJ
    rt.lib.touched = 24
    dms = _dofmaps(gather.capacity + 1)
    first = [gather.get(dm, 24)[0] for dm in dms[:-1]]
    assert rt.lib.released() == []
    gather.get(dms[-1], 24)
    assert rt.lib.released() == [first[0].data_ptr()]
    detJ = [torch.ones((3, 8), dtype=torch.float64) for _ in range(static.capacity + 1)]
    held = [static.get(first[1], d, 8, 3)[0] for d in detJ]
    assert rt.lib.released() == [first[0].data_ptr(), held[0].data_ptr()]
    assert len(static._entries) == static.capacity


def test_a_refused_entry_is_evicted_without_a_release(rt):
    gather = rt.ops._GATHER_PLANS
    rt.lib.touched = 24
    rt.lib.refuse.add("fus_mass_gather_plan_build")
    dms = _dofmaps(gather.capacity + 1)
    assert gather.get(dms[0], 24) is None
    rt.lib.refuse.clear()
    for dm in dms[1:]:
        assert gather.get(dm, 24) is not None
    assert rt.lib.released() == []


def _fill_all_three(rt):
    rt.lib.touched = 18000
    args = _mass_args(27, 2000, 18000)
    rt.ops.mass_operator(27, np.float64, static_detJ=True)(*args)
    rt.ops.mass_operator(27, np.float64)(*args)
    (plan,), (gather,), (static,) = rt.ops._PLANS._plans.values(), _entries(rt.ops._GATHER_PLANS).values(), rt.ops._STATIC_DETJ._entries.values()
    return args, [plan[0], gather[0], static[0]]


def _entries(cache):
    return cache._entries if hasattr(cache, "_entries") else cache._plans


def test_clear_empties_the_dependent_caches(rt):
    ops = rt.ops
    _, (plan, gather, static) = _fill_all_three(rt)
    ops._PLANS.clear()
    assert sorted(rt.lib.released()) == sorted(t.data_ptr() for t in (plan, gather, static))  # every workspace, once
    assert not ops._PLANS._plans and not _entries(ops._GATHER_PLANS) and not ops._STATIC_DETJ._entries
    rt.lib.raw.clear()
    _, (plan, gather, static) = _fill_all_three(rt)
    ops._GATHER_PLANS.clear()
    assert sorted(rt.lib.released()) == sorted(t.data_ptr() for t in (gather, static))
    assert len(ops._PLANS._plans) == 1 and not _entries(ops._GATHER_PLANS) and not ops._STATIC_DETJ._entries
    rt.lib.raw.clear()
    ops._STATIC_DETJ.clear()
    ops._GATHER_PLANS.clear()
    assert rt.lib.released() == []


def test_hits_between_start_and_stop_recording_are_held(rt):
    ops = rt.ops
    args, workspaces = _fill_all_three(rt)
    assert ops._PLANS.stop_recording() == []  # not recording: nothing held
    ops._PLANS.start_recording()
    ops.mass_operator(27, np.float64, static_detJ=True)(*args)
    ops.mass_operator(27, np.float64)(*args)
    held = ops._PLANS.stop_recording()
    got = {t.data_ptr() for pair in held for t in pair}
    assert {w.data_ptr() for w in workspaces} <= got
    assert {args[4].data_ptr(), args[3].data_ptr()} <= got  # ... with the dofmap and the detJ array their keys name
    ops.mass_operator(27, np.float64)(*args)
    assert ops._PLANS.stop_recording() == []


def test_cache_keys_follow_the_identity_of_the_dofmap(rt):
    ops = rt.ops
    rt.lib.touched = 18750
    args = _mass_args(125, 300, 18750)
    dm = args[4]
    ops._PLANS.get(dm)
    ops._GATHER_PLANS.get(dm, 18750)
    rt.lib.take()
    assert ops._PLANS.get(dm)[1] == EPB and ops._GATHER_PLANS.get(dm, 18750)[2][0] == 18750
    assert rt.lib.take() == []  # a second get with the same dofmap builds nothing
    dm.add_(0)  # torch's version counter moves
    assert not ops._PLANS.has(dm)
    ops._PLANS.get(dm)
    ops._GATHER_PLANS.get(dm, 18750)
    assert rt.lib.take() == PLAN_SETUP + GATHER_SETUP
    ops._GATHER_PLANS.get(dm, 18751)  # the gather plan is also keyed on the length of the dof vectors
    assert rt.lib.take() == GATHER_SETUP
    detJ = args[3]
    plan = ops._GATHER_PLANS.get(dm, 18750)
    ops._STATIC_DETJ.get(plan[0], detJ, 125, 300)
    ops._STATIC_DETJ.get(plan[0], detJ, 125, 300)
    assert rt.lib.take() == STATIC_SETUP
    detJ.mul_(1.0)
    ops._STATIC_DETJ.get(plan[0], detJ, 125, 300)
    assert rt.lib.take() == STATIC_SETUP


def test_vector_ops_and_diagonal_mass(rt):
    ops = rt.ops
    a, b, c = (torch.zeros(7, dtype=torch.float32) for _ in range(3))
    ops.axpy(5)(2.0, a, b)
    ops.axpy[1, 1](2.0, a, b)
    ops.scale(2.0, a, b)
    ops.copy(a, b)
    ops.fill[1, 1](1.0, a)
    ops.pointwise_divide(a, b, c)
    ops.square(a, b)
    assert rt.lib.take() == [f"fus_{n}_f32" for n in ("axpy", "axpy", "scale", "copy", "fill", "pointwise_divide", "square")]
    assert [c_[1][-2] for c_ in rt.lib.last] == [5, 7, 7, 7, 7, 7, 7]
    with pytest.raises(ValueError):
        ops.axpy(8)(2.0, a, b)
    with pytest.raises(TypeError):
        ops.copy(a, b.double())
    x, cc, y, detJ, dm = _mass_args(125, 10, 1000)
    d = ops.diagonal_mass_operator(cc, detJ, dm, 1000)
    d(x, y)
    assert rt.lib.take() == ["fus_mass_apply_f64", "fus_muladd_f64"]
