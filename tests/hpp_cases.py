"""The cases of tests/host/fus_gpu_hpp_run.cpp (the driver that runs every functor of include/fus_gpu.hpp on the device) and their fp64
models, for tests/test_fus_gpu_hpp_gpu.py; what that test takes for granted about them is checked in tests/test_hpp_cases.py.

A case file is the container of tests/golden/export_raw.py (``FUSGOLD1``: named entries of float64 / int32 / int64).  Every entry is
named ``<group>.<array>``; the driver runs the groups it finds and writes every output array, widened to float64, into a file of the
same format.  Floating-point inputs are stored as float64 and hold values that are exact in the case's type, so the driver narrows
them without loss and the models below read what the device holds.

A group is ``Group(name, inputs, model, swaps)``: ``model(inputs)`` returns ``{output: Check}`` -- the expected array in fp64 and the
bar it is held to -- and is assembled from the models the suite already has:

    cell       cell_model64 (box, factors' precompute, the C oracle's applies), gradient_cpu.weak_gradient, nodal_cpu.stiffness_apply,
               westervelt_nodal_cpu.stiffness_pair; the inputs are those of cell_model64 / nodal_model64's cases        conftest.TOL
    colliding  cell_model64.colliding with cell_model64.stiffness("general") / mass("mass")                              conftest.TOL
    declined   one dof in 300 cells (P = 1): the oracle's mass apply                                                     conftest.TOL
    probe      numpy, as tests/test_sensors_gpu.py: values 1e-13 / 1e-5 of the largest; peaks bitwise against the rows
    psource    point_source_cpu.inject of sources._waveform                                                             conftest.TOL
    facet      facet_cpu.reference64 / facet_sets / dof_bound (+ evaluation_slack in fp64, as tests/test_small_kernels_gpu.py)
    receive    point_source_cpu.receive                                                   conftest.TOL; the two runs bitwise
    monitor    numpy, as tests/test_field_monitor_gpu.py: extrema bitwise, sums 2 K eps64 sum |terms|
    bioheat    bioheat_cpu.stage_reference: 8 eps sum |terms|, the dose 4 eps64 against the rule on the kernel's own T
    relax      test_relaxation_gpu._numpy_stage: 16 eps max(1, max |ref|)
    loop       bioheat_cpu.CpuBioheat.advance, three steps at P = 4                tests/test_bioheat_gpu.py::_check_against_cpu

The two stage functors take the stage index; ``bw``, ``aw`` and ``kind`` of the models come from the package's own tableau
(``solver_base.A_RUNGE`` / ``B_RUNGE``), not from the header.

``swaps`` lists the groups of same-typed pointer arguments a forward of the header could exchange and the outputs each exchange must
change (a tuple of outputs: at least one of them): ``exchanged(group, a, b)`` is the model of the launch with the two pointers exchanged (inputs exchanged before, outputs of those
names after).  CPU only; not a test module."""

import struct
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import bioheat_cpu
import cell_model64 as cm
import facet_cpu
import gradient_cpu
import nodal_cpu
import nodal_model64
import point_source_cpu
import westervelt_nodal_cpu
from conftest import TOL, pkg

MAGIC = b"FUSGOLD1"
CODES = {np.dtype(np.float64): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2}  # tests/golden/export_raw.py
DTYPES = {"double": np.float64, "float": np.float32}
SENTINEL = -7.25
DEGREES = tuple(range(1, 11))
LN4 = float(np.log(4.0))
EPS64 = float(np.finfo(np.float64).eps)

# kind: "tol" (conftest.TOL: rel l2 and rel max), "abs" (|got - ref| <= bound per entry), "bits" (equal to ref), "same" (equal to the
# output named ``ref``), "own" (``ref(got, inputs)`` -> (error, bound) arrays formed from the driver's own outputs)
Check = namedtuple("Check", "kind ref bound", defaults=(None,))
Group = namedtuple("Group", "name inputs model swaps")


# ---- the container ---------------------------------------------------------------------------------------------------------------------
def encode(entries):
    out = [MAGIC, struct.pack("<q", len(entries))]
    for name, a in entries.items():
        a = np.ascontiguousarray(a)
        assert a.dtype in CODES and len(name.encode()) < 32, (name, a.dtype)
        raw = a.tobytes()
        out.append(name.encode().ljust(32, b"\0"))
        out.append(struct.pack("<iiq", CODES[a.dtype], 0, a.size))
        out.append(raw + b"\0" * (-len(raw) % 8))
    return b"".join(out)


def decode(blob):
    assert blob[:8] == MAGIC
    (n,), at, out = struct.unpack_from("<q", blob, 8), 16, {}
    kinds = {v: k for k, v in CODES.items()}
    for _ in range(n):
        name = blob[at:at + 32].rstrip(b"\0").decode()
        code, _, count = struct.unpack_from("<iiq", blob, at + 32)
        dt = kinds[code]
        out[name] = np.frombuffer(blob, dtype=dt, count=count, offset=at + 48).copy()
        at += 48 + -(-count * dt.itemsize // 8) * 8
    assert at == len(blob)
    return out


def write_case(path, groups):
    entries = {}
    for g in groups:
        for k, a in g.inputs.items():
            a = np.asarray(a)
            entries[f"{g.name}.{k}"] = a.astype(np.float64) if a.dtype.kind == "f" else a
    with open(path, "wb") as f:
        f.write(encode(entries))


def read_outputs(path, group):
    with open(path, "rb") as f:
        d = decode(f.read())
    return {k[len(group) + 1:]: v for k, v in d.items() if k.startswith(group + ".")}


def exchanged(group, a, b):
    """The model of the launch with the pointers ``a`` and ``b`` exchanged."""
    inp = dict(group.inputs)
    if a in inp and b in inp:
        inp[a], inp[b] = inp[b], inp[a]
    out = dict(group.model(inp))
    if a in out and b in out:
        out[a], out[b] = out[b], out[a]
    return out


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i1(v):
    return np.array([v], dtype=np.int64)


# ---- the cell functors on the perturbed (3, 2, 2) box -------------------------------------------------------------------------------------
def cell_group(P, dtype):
    """Mass and Stiffness through ``Geometry<T>``, Gradient, Nodal and WesterveltNodal on ``cell_model64.box(P, (3, 2, 2))``."""
    gll, pre = pkg("gll"), pkg("precompute")
    geo = cm.box(P, (3, 2, 2), dtype)
    nd, nc, dm = geo["ndofs"], geo["ncells"], geo["dofmap"]
    st, gr, no, pa, ma = cm.stiffness("geom", geo), cm.gradient("gradient", geo), nodal_model64.stiffness(geo), nodal_model64.pair(geo), cm.mass("mass", geo)
    ystride = nd + 5
    inputs = dict(P=_i1(P), ndofs=_i1(nd), x_g=geo["x_g"], x_dofs=geo["x_dofs"], dofmap=dm, pts=geo["pts"], wts=geo["wts"], dphi=geo["D"],
                  dphi_p1=pre.tabulate_hex_p1_gradients(gll.tensor_points_3d(geo["pts"]), dtype), w3=gll.tensor_weights_3d(geo["wts"]).astype(dtype),
                  cc=geo["cc"], xs=st["x"], ys0=st["out"]["y"]["y0"], xm=ma["x"], ym0=ma["out"]["y"]["y0"], xg=gr["x"],
                  yg0=np.stack([gr["out"][k]["y0"] for k in cm.COMPONENTS]), ystride=_i1(ystride), xn=no["x"], nodal=no["kappa"], yn0=no["y0"],
                  u=pa["u"], v=pa["v"], nodal3=pa["k3"], nodal4=pa["k4"], c3=pa["c3"], c4=pa["c4"], b0=pa["y0"])

    def model(i):
        f = {k: _f64(a) for k, a in i.items() if np.asarray(a).dtype.kind == "f"}
        mesh = (i["x_dofs"], f["x_g"])
        G, detJ = np.zeros((nc, (P + 1) ** 3, 6)), np.zeros((nc, (P + 1) ** 3))
        pre.compute_scaled_geometrical_factor(G, mesh, nc, f["dphi_p1"], f["w3"])
        pre.compute_scaled_jacobian_determinant(detJ, mesh, nc, f["dphi_p1"], f["w3"])
        orc = cm.oracle()
        ys, ym = f["ys0"].copy(), f["ym0"].copy()
        orc.stiffness_apply(P, f["dphi"], f["xs"], f["cc"], ys, G, dm)
        orc.mass_apply(f["xm"], f["cc"], ym, detJ, dm)
        # the three kernels that form the geometry themselves, from the 1-D rule
        geo1 = dict(geo, pts=f["pts"], wts=f["wts"], x_g=f["x_g"])
        G1 = nodal_model64.factors64(geo1)
        g3 = gradient_cpu.weak_gradient(i["x_dofs"], f["x_g"], f["pts"], f["wts"], f["dphi"], dm, f["xg"], f["cc"], nd)
        yg = np.full((3, ystride), SENTINEL)
        yg[:, :nd] = f["yg0"] + g3
        yn, b = f["yn0"].copy(), f["b0"].copy()
        nodal_cpu.stiffness_apply(P, f["dphi"], f["xn"], f["cc"], yn, G1, dm, f["nodal"])
        westervelt_nodal_cpu.stiffness_pair(P, f["dphi"], f["u"], f["v"], f["c3"], f["c4"], b, G1, dm, f["nodal3"], f["nodal4"])
        out = dict(G=Check("tol", G.reshape(-1)), stiff=Check("tol", ys), mass_op=Check("tol", ym), mass_atomic=Check("tol", ym),
                   mass_gather=Check("tol", ym), mass_static=Check("tol", ym), mass_static_same=Check("same", "mass_gather"),
                   nodal=Check("tol", yn), wnodal=Check("tol", b), grad_pad=Check("bits", yg[:, nd:].reshape(-1)),
                   flags=Check("bits", np.array([0.0, 0.0, 1.0, 0.0, 1.0, 1.0])))  # gather / static: before, static off, default
        for d, k in enumerate(cm.COMPONENTS):
            out["grad_" + k] = Check("tol", yg[d, :nd])
        return out

    grads = tuple("grad_" + k for k in cm.COMPONENTS)
    swaps = [(("pts", "wts"), grads + ("nodal", "wnodal")), (("nodal3", "nodal4"), ("wnodal",)), (("c3", "c4"), ("wnodal",))]
    g = Group("cell", inputs, model, swaps)
    for rec, k in ((st["out"]["y"], "stiff"), (no, "nodal"), (pa, "wnodal")):  # the suite's own cases say the same
        assert np.max(np.abs(model(inputs)[k].ref - rec["ref"])) <= 1e-5 * np.max(np.abs(rec["ref"]))
    return g


def colliding_group(P, dtype):
    """Stiffness and Mass on caller-owned factors: the 37-cell colliding dofmap of ``cell_model64.colliding``."""
    geo = cm.colliding(dtype, P=P)
    st, ma = cm.stiffness("general", geo), cm.mass("mass", geo)
    inputs = dict(ndofs=_i1(geo["ndofs"]), dofmap=geo["dofmap"], G=geo["G"], detJ=geo["detJ"], cc=geo["cc"], dphi=geo["D"], xs=st["x"],
                  ys0=st["out"]["y"]["y0"], xm=ma["x"], ym0=ma["out"]["y"]["y0"])

    # the gather plan takes at most 255 entries per dof: from P = 6 on this dofmap is declined and every apply is the atomic kernel's
    ok = float(np.bincount(geo["dofmap"].reshape(-1)).max() <= 255)
    flags = np.array([ok, 0.0, ok, ok, ok, ok])  # gather / static after: the default, kStaticAlways, enable_gather again

    def model(i):
        ym = Check("tol", ma["out"]["y"]["ref"])
        out = dict(stiff=Check("tol", st["out"]["y"]["ref"]), mass_atomic=ym, mass_gather=ym, mass_static=ym, mass_again=ym, flags=Check("bits", flags))
        if ok:  # (the atomic kernel's sums depend on the order of its adds)
            out.update(mass_static_same=Check("same", "mass_gather"), mass_again_same=Check("same", "mass_gather"))
        return out

    return Group("coll", inputs, model, [])


def declined_group(dtype, ncells=300, ndofs=700):
    """P = 1: dof 0 is a vertex of every one of 300 cells, more than the 255 the gather plan takes: ``enable_gather`` leaves the functor
    on the atomic kernel."""
    rng = np.random.default_rng([91, np.dtype(dtype).itemsize])
    dm = rng.integers(1, ndofs, (ncells, 8)).astype(np.int32)
    dm[:, 0] = 0
    detJ, cc = rng.uniform(0.5, 1.5, (ncells, 8)).astype(dtype), (1.0 + 0.25 * rng.standard_normal(ncells)).astype(dtype)
    x = rng.standard_normal(ndofs).astype(dtype)
    add = np.zeros(ndofs)
    cm.oracle().mass_apply(_f64(x), _f64(cc), add, _f64(detJ), dm)
    y0 = (0.1 * np.sqrt(np.mean(add**2)) * rng.standard_normal(ndofs)).astype(dtype)
    inputs = dict(ndofs=_i1(ndofs), dofmap=dm, detJ=detJ, cc=cc, x=x, y0=y0)
    return Group("decl", inputs, lambda i: dict(mass=Check("tol", _f64(y0) + add), flags=Check("bits", np.array([0.0, 0.0]))), [])


# ---- probe and point source: about 300 points on the same box --------------------------------------------------------------------------
def _points(P, dtype, rng, npts=300):
    """cells [npts] and weights [npts][3][P + 1] of points at random reference coordinates of random cells of the (3, 2, 2) box: points
    0 and 1 coincide, point 2 lies on a cell vertex (one-hot rows)."""
    sens, gll = pkg("sensors"), pkg("gll")
    geo = nodal_model64.box(P, (3, 2, 2), dtype)
    cells = np.sort(rng.integers(0, geo["ncells"], npts)).astype(np.int32)
    xi = rng.uniform(0.0, 1.0, (npts, 3))
    cells[1], xi[1] = cells[0], xi[0]
    xi[2] = (1.0, 0.0, 1.0)
    nodes, _ = gll.gll_points_weights(P)
    w = np.stack([sens._lagrange_1d(nodes, xi[:, a]) for a in range(3)], axis=1).astype(dtype)
    assert np.array_equal(np.sort(np.abs(w[2]), axis=1)[:, -1], np.ones(3)) and not np.any(np.sort(np.abs(w[2]), axis=1)[:, :-1])
    return geo, cells, w


def _tensor_weights(w):
    w = _f64(w)
    return (w[:, 0, :, None, None] * w[:, 1, None, :, None] * w[:, 2, None, None, :]).reshape(w.shape[0], -1)


def probe_group(P, dtype):
    """The short form on three fields; the general form three times into slot 2 of 4 with peaks and H = 2 harmonic sums."""
    rng = np.random.default_rng([92, P, np.dtype(dtype).itemsize])
    geo, cells, w = _points(P, dtype, rng)
    npts, nd, K, H = cells.size, geo["ndofs"], 3, 2
    u = (1e3 * rng.standard_normal((K, nd))).astype(dtype)
    coef = np.array([[0.9, -0.3, 0.45, 0.7], [-0.8, 0.55, 0.25, -0.65], [0.35, 0.95, -0.6, 0.15]]).astype(dtype)
    inputs = dict(P=_i1(P), cells=cells, dofmap=geo["dofmap"], weights=w, u=u, coef=coef, pmax=np.full(npts, -np.inf), pmin=np.full(npts, np.inf),
                  hre=np.zeros((H, npts)), him=np.zeros((H, npts)))
    tolv = 1e-13 if dtype == np.float64 else 1e-5  # tests/test_sensors_gpu.py::test_device_evaluation_matches_eval_function

    def model(i):
        W, c, uu = _tensor_weights(i["weights"]), _f64(i["coef"]), _f64(i["u"])
        vals = np.stack([np.sum(W * uu[k][i["dofmap"][i["cells"]]], axis=1) for k in range(K)])
        bound = np.full(npts, tolv * np.max(np.abs(vals)))
        rec = np.full((4, npts), SENTINEL)
        rec[2] = vals[K - 1]
        out = {f"short{k}": Check("abs", vals[k], bound) for k in range(K)}
        out.update(rec_row=Check("abs", rec[2], bound), rec_rest=Check("bits", rec[[0, 1, 3]].reshape(-1)),
                   pmax=Check("abs", np.maximum(_f64(i["pmax"]), vals.max(axis=0)), bound), pmin=Check("abs", np.minimum(_f64(i["pmin"]), vals.min(axis=0)), bound))
        for name, off in (("hre", 0), ("him", 1)):  # a sum of K products in double; the values carry the type's rounding
            ref = _f64(i[name]) + np.stack([sum(vals[k] * c[k, 2 * h + off] for k in range(K)) for h in range(H)])
            mag = np.stack([sum(np.abs(c[k, 2 * h + off]) for k in range(K)) * bound for h in range(H)])
            out[name] = Check("abs", ref.reshape(-1), mag.reshape(-1))
        # against the driver's own rows: the peaks to the bit, the sums to 2 K eps64 sum |terms|
        rows = lambda got: np.stack([got[f"short{k}"] for k in range(K)])  # noqa: E731
        zero = np.zeros(npts)
        out["pmax_own"] = Check("own", lambda got, i: (np.abs(got["pmax"] - rows(got).max(axis=0)), zero))
        out["pmin_own"] = Check("own", lambda got, i: (np.abs(got["pmin"] - rows(got).min(axis=0)), zero))
        out["rec_own"] = Check("own", lambda got, i: (np.abs(got["rec_row"] - got[f"short{K - 1}"]), zero))

        def harmonic(name, off):
            def f(got, i):
                r = rows(got)
                ref = np.stack([sum(r[k] * c[k, 2 * h + off] for k in range(K)) for h in range(H)])
                mag = np.stack([sum(np.abs(r[k] * c[k, 2 * h + off]) for k in range(K)) for h in range(H)])
                return np.abs(got[name].reshape(H, npts) - ref).reshape(-1), (2 * K * EPS64 * mag).reshape(-1)
            return f
        out["hre_own"], out["him_own"] = Check("own", harmonic("hre", 0)), Check("own", harmonic("him", 1))
        return out

    return Group("probe", inputs, model, [(("pmax", "pmin"), ("pmax", "pmin")), (("hre", "him"), ("hre", "him"))])


F0 = 2.0**19  # the carrier of the source cases: the period is exact in either type
T0 = 1.0 / F0


def psource_group(P, dtype):
    """One stage block at t = 12.3 T of a burst of 12 T; the delays put a quarter of the points each before their start, on the ramp, on
    the plateau and after the burst (tests/test_point_sources_gpu.py::test_point_source_kernel)."""
    src = pkg("sources")
    rng = np.random.default_rng([93, P, np.dtype(dtype).itemsize])
    geo, cells, w = _points(P, dtype, rng)
    npts, nd, n = cells.size, geo["ndofs"], P + 1
    r = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)  # noqa: E731
    delay = np.array([13 * T0, 11 * T0, 5 * T0, 0.0])[(np.arange(npts) + 2) % 4]
    delay[:3] = 5 * T0  # the coincident pair and the vertex point fire
    # amplitude, phase and delay on ranges that do not meet, all of them sizes a burst responds to: amplitudes 0.5 .. 2, phases -3 .. -2.2
    amplitude, phase = r(rng.uniform(0.5, 2.0, npts)), r(rng.uniform(-3.0, -2.2, npts))
    stage = r([12.3 * T0, 2.0 * np.pi * F0, 1.75, F0, 4.0, 12 * T0])
    y0 = (rng.uniform(0.5, 2.0, nd) * rng.choice([-1.0, 1.0], nd)).astype(dtype)
    inputs = dict(P=_i1(P), cells=cells, dofmap=geo["dofmap"], weights=w, amplitude=amplitude, phase=phase, delay=r(delay), stage=stage, y0=y0)
    uniq, cell_index = np.unique(cells, return_inverse=True)

    def model(i):
        t, w0, A, f0, alpha, D = _f64(i["stage"])
        g, _ = src._waveform(t, f0, A, _f64(i["amplitude"]), _f64(i["phase"]), _f64(i["delay"]), D, alpha)
        setup = SimpleNamespace(point_ids=np.arange(npts), weights=_f64(i["weights"]), rows=i["dofmap"][uniq], cell_index=cell_index.reshape(-1))
        return dict(y=Check("tol", point_source_cpu.inject(_f64(i["y0"]).copy(), setup, g, n)))

    s = float(stage[0]) - r(delay)
    assert np.any(s < 0) and np.any((s > 0) & (s < 4 * T0)) and np.any((s > 4 * T0) & (s < 8 * T0)) and np.any(s > 12 * T0)
    return Group("psrc", inputs, model, [(("amplitude", "phase", "delay"), ("y",))])


# ---- the degree-free functors -------------------------------------------------------------------------------------------------------------
def facet_group(dtype, N=9, nA=300, nB=170, ndofs=5000, E=23):
    """``operator()`` and ``device_stage`` with c2 and a set B whose ``xB`` is null (nothing of B may be added); without c2 and with xB."""
    src = pkg("sources")
    rng = np.random.default_rng([94, np.dtype(dtype).itemsize])
    r = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)  # noqa: E731
    eid = rng.integers(-1, E, nA).astype(np.int32)
    delay = np.concatenate([[15.0 * T0, 13.5 * T0, 12.0 * T0, 8.0 * T0, 3.5 * T0, 1.0 * T0, 0.0], 11.0 * T0 * rng.random(E - 7) + T0])
    amplitude, phase, delay = r(0.5 + rng.random(E)), r(-3.0 + 0.8 * rng.random(E)), r(delay)
    stage = r([14.0 * T0, 2.0 * np.pi * F0, 1.75, F0, 4.0, 12 * T0])
    s = facet_cpu.facet_sets(rng, dtype, N, nA, nB, ndofs)
    # c2 multiplies dg = O(w0 g): at 1e-6 .. 2e-6 its term is as large as c1's (an exchange of c1 and c2 is then an O(1) change)
    s["c2"] = (1e-6 * (1.0 + rng.random(nA))).astype(dtype)
    y0 = rng.standard_normal(ndofs).astype(dtype)
    inputs = dict(N=_i1(N), c1=s["c1"], c2=s["c2"], detJ=s["dA"], dofmap=s["dmA"], eid=eid, amplitude=amplitude, phase=phase, delay=delay, stage=stage,
                  xB=s["x"], cB=s["cB"], detJB=s["dB"], dmB=s["dmB"], y0=y0)

    def model(i):
        t, w0, A, f0, alpha, D = _f64(i["stage"])
        g, dg = src._waveform(t, f0, A, _f64(i["amplitude"]), _f64(i["phase"]), _f64(i["delay"]), D, alpha)
        e, act = np.maximum(i["eid"], 0), i["eid"] >= 0
        c1, c2, dA = _f64(i["c1"]), _f64(i["c2"]), _f64(i["detJ"])
        v1, v2 = np.where(act, g[e], 0.0) * c1, np.where(act, dg[e], 0.0) * c2
        eg, edg = facet_cpu.evaluation_slack(SimpleNamespace(amplitude=_f64(i["amplitude"]), waveform=None), f0, A)
        out = {}
        for name, vv2, field in (("with_c2", v2, None), ("no_c2", None, (i["xB"], i["cB"], i["detJB"], i["dmB"]))):
            ref, mag, k = facet_cpu.reference64(i["y0"], v1, vv2, dA, i["dofmap"], field)
            bound = facet_cpu.dof_bound(mag, k, dtype)
            if dtype == np.float64:  # two fp64 evaluations of g_e (tests/test_small_kernels_gpu.py::_evaluation_slack)
                per = eg[e] * np.abs(c1) + (edg[e] * np.abs(c2) if vv2 is not None else 0.0)
                live = v1 != 0
                np.add.at(bound, i["dofmap"][live].reshape(-1), (per[live, None] * np.abs(dA)[live]).reshape(-1))
            out[name] = Check("abs", ref, bound)
        out["with_c2_dev"] = out["with_c2"]
        return out

    return Group("facet", inputs, model, [(("amplitude", "phase", "delay"), ("with_c2", "no_c2")), (("c1", "c2"), ("with_c2",))])


def receive_group(dtype, ndofs=2000):
    """Elements with no entry, one entry, more than 1024 entries (the unrolled loop and its tail) and a few more; two launches into slot
    1 of 3 of two record buffers, the second with other factors, H = 2."""
    rng = np.random.default_rng([95, np.dtype(dtype).itemsize])
    counts = np.array([0, 1, 1027, 64, 0, 301, 6])
    E, total = counts.size, int(counts.sum())
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    dof, wgt = rng.integers(0, ndofs, total).astype(np.int32), rng.uniform(0.1, 1.0, total).astype(dtype)
    u = (1e3 * rng.standard_normal(ndofs)).astype(dtype)
    coef = np.array([[0.9, -0.3, 0.45, 0.7], [-0.8, 0.55, 0.25, -0.65]]).astype(dtype)
    inputs = dict(dof=dof, wgt=wgt, offsets=offsets, u=u, coef=coef, hre=np.zeros((2, E)), him=np.zeros((2, E)))
    ids = np.repeat(np.arange(E), counts)

    def model(i):
        S, _ = point_source_cpu.receive(_f64(i["u"]), ids, i["dof"][:, None], _f64(i["wgt"])[:, None], E)
        c = _f64(i["coef"])
        rest = np.full(2 * E, SENTINEL)
        out = dict(rec1=Check("tol", S), rec2=Check("same", "rec1"), rest1=Check("bits", rest), rest2=Check("bits", rest))
        for name, off in (("hre", 0), ("him", 1)):
            ref = _f64(i[name]) + np.stack([S * (c[0, 2 * h + off] + c[1, 2 * h + off]) for h in range(2)])
            out[name] = Check("tol", ref.reshape(-1))
            # tests/test_receivers_gpu.py: the sums against the kernel's own series, to 1e-14
            out[name + "_own"] = Check("own", lambda got, i, name=name, off=off: (
                np.abs(got[name].reshape(2, E) - np.stack([got["rec1"] * c[0, 2 * h + off] + got["rec2"] * c[1, 2 * h + off] for h in range(2)])).reshape(-1),
                np.full(2 * E, 1e-14 * np.max(np.abs(got["rec1"])))))
        return out

    return Group("recv", inputs, model, [(("hre", "him"), ("hre", "him"))])


N_LOCAL, N_TOTAL = 997, 1003  # the streaming functors: an odd count inside a longer row


def monitor_group(dtype, K=3, H=2):
    """Three records of (u, v), the first with ``init``; H = 2 with hstride = 1003 > n = 997; every output starts as the sentinel."""
    rng = np.random.default_rng([96, np.dtype(dtype).itemsize])
    n = N_LOCAL
    u, v = (10.0 * rng.standard_normal((K, n))).astype(dtype), (1e3 * rng.standard_normal((K, n))).astype(dtype)
    coef = np.array([[0.9, -0.3, 0.45, 0.7], [-0.8, 0.55, 0.25, -0.65], [0.35, 0.95, -0.6, 0.15]]).astype(dtype)
    inputs = dict(u=u, v=v, coef=coef)

    def sums(terms):  # tests/test_field_monitor_gpu.py::_window
        acc = terms[0].copy()
        for k in range(1, K):
            acc = acc + terms[k]
        return Check("abs", acc, 2 * K * EPS64 * np.abs(terms).sum(axis=0))

    def model(i):
        U, V, c = _f64(i["u"]), _f64(i["v"]), _f64(i["coef"])
        out = dict(pmax=Check("bits", U.max(axis=0)), pmin=Check("bits", U.min(axis=0)), usq=sums(U * U), vsq=sums(V * V),
                   pad=Check("bits", np.full(2 * H * (int(i["hstride"][0]) - n), SENTINEL)))
        for name, off in (("hre", 0), ("him", 1)):
            per = [sums(U * c[:, 2 * h + off][:, None]) for h in range(H)]
            out[name] = Check("abs", np.concatenate([p.ref for p in per]), np.concatenate([p.bound for p in per]))
        return out

    swaps = [(("pmax", "pmin"), ("pmax", "pmin")), (("hre", "him"), ("hre", "him")), (("usq", "vsq"), ("usq", "vsq"))]
    # 16-byte aligned with an even hstride (the 16-byte access path); sliced one element in with an odd one (the scalar path)
    return [Group(name, dict(inputs, hstride=_i1(hs)), model, swaps) for name, hs in (("mon_a", N_TOTAL + 1), ("mon_s", N_TOTAL))]


def tableau(i, dt, dtype):
    """(bw, aw, kind) of stage ``i`` as the Python solvers hand them to the stage kernels, from the package's tableau, in the field's type."""
    sb = pkg("solver_base")
    bw, aw = sb.B_RUNGE[i] * dt, 0.0 if i == 3 else sb.A_RUNGE[i + 1] * dt
    return float(dtype(bw)), float(dtype(aw)), 2 if i == 3 else (0 if i == 0 else 1)


BIOHEAT_RUNS = [(f"{v}{i}", i, v) for i in range(4) for v in ("full", "bare")] + [("init3", 3, "init")]


def bioheat_group(dtype):
    """Stages 0 .. 3 on random operands (tests/test_bioheat_gpu.py::_stage_case): with pr, s, cem43 and tmax (``full``), without any of
    them (``bare``), and stage 3 with ``init``.  Every run starts from the same operands."""
    rng = np.random.default_rng([97, np.dtype(dtype).itemsize])
    eps = float(np.finfo(dtype).eps)
    r = lambda lo, hi, n=N_TOTAL: rng.uniform(lo, hi, n).astype(dtype)  # noqa: E731
    n = N_LOCAL
    inputs = dict(minv=r(0.5, 2.0), b=r(-3.0, 3.0), T0=r(36.0, 50.0), Tn=r(36.0, 50.0), acc=r(36.0, 50.0), pr=r(0.6, 0.9), s=r(2.5, 4.0),
                  tmax=r(36.0, 50.0, n), cem43=np.asarray(rng.uniform(0.0, 30.0, n), dtype=dtype).astype(np.float64),
                  scalars=np.asarray([0.37, 0.7, 37.0], dtype=dtype).astype(np.float64), nlocal=_i1(n))

    def model(i):
        f = {k: _f64(a) for k, a in i.items()}
        dt, gate, Ta = f["scalars"]
        out = {}
        for tag, st, variant in BIOHEAT_RUNS:
            bw, aw, kind = tableau(st, dt, dtype)
            on, init = variant != "bare", variant == "init"
            ref, terms = bioheat_cpu.stage_reference(kind, bw, aw, gate, Ta, dt, *(f[k][:n] for k in ("minv", "b", "T0", "Tn", "acc")),
                                                     pr=f["pr"][:n] if on else None, s=f["s"][:n] if on else None,
                                                     cem43=f["cem43"] if (on and kind == 2) else None, init=init)
            for name in ("T0", "Tn", "acc"):
                full, bound = f[name].copy(), np.zeros(N_TOTAL)  # what the stage does not write, the ghost entries among it, keeps its bits
                if name in ref:
                    full[:n], bound[:n] = ref[name], 8 * eps * terms[name]
                out[f"{tag}.{name}"] = Check("abs", full, bound)
            out[f"{tag}.b"] = Check("bits", np.zeros(N_TOTAL))
            if kind == 2 and on:
                out[f"{tag}.tmax"] = Check("own", lambda got, i, tag=tag, init=init: (
                    np.abs(got[f"{tag}.tmax"] - (got[f"{tag}.T0"][:n] if init else np.maximum(f["tmax"], got[f"{tag}.T0"][:n]))), np.zeros(n)))
                out[f"{tag}.cem43"] = Check("own", lambda got, i, tag=tag, init=init, Tref=ref["T0"], cref=ref["cem43"]: (
                    np.abs(got[f"{tag}.cem43"] - cref), (LN4 * np.abs(got[f"{tag}.T0"][:n] - Tref) + 4 * eps) * cref))

                def own_dose(got, i, tag=tag, init=init):
                    own = bioheat_cpu.dose_increment(got[f"{tag}.T0"][:n], dt) + (0.0 if init else f["cem43"])
                    return np.abs(got[f"{tag}.cem43"] - own), 4 * EPS64 * own
                out[f"{tag}.dose"] = Check("own", own_dose)
            else:
                out[f"{tag}.tmax"], out[f"{tag}.cem43"] = Check("bits", f["tmax"]), Check("bits", f["cem43"])
        return out

    # per run one set of outputs, of which an exchange must move at least one (a stage leaves one or two of its vectors unwritten)
    states = tuple(tuple(f"{tag}.{name}" for name in ("T0", "Tn", "acc")) for tag, _, _ in BIOHEAT_RUNS)
    full = tuple(k for k in states if not k[0].startswith("bare"))
    return [Group(name, inputs, model, [(("minv", "pr", "s"), full), (("T0", "Tn", "acc"), states)]) for name in ("bio_a", "bio_s")]


RELAX_RUNS = [(f"n{nr}{'d' if perdof else 's'}{i}", nr, perdof, i) for nr in (1, 4) for perdof in (True, False) for i in range(4)]


def relax_group(dtype):
    """Stages 0 .. 3 with nr = 1 and nr = 4, per-dof ``kappa`` and a null ``kappa`` with ``kappa_scalar``
    (tests/test_relaxation_gpu.py::_relax_stage_launches).  Every run starts from the same state."""
    from test_relaxation_gpu import _numpy_stage

    rng = np.random.default_rng([98, np.dtype(dtype).itemsize])
    eps = float(np.finfo(dtype).eps)
    n, stride = N_LOCAL, N_TOTAL
    signed = lambda: (rng.uniform(0.5, 2.0, (4, stride)) * rng.choice([-1.0, 1.0], (4, stride))).astype(dtype)  # noqa: E731
    inputs = dict(tau=np.asarray(rng.uniform(0.5, 2.0, 4), dtype=dtype).astype(np.float64), ks=np.asarray(rng.uniform(0.2, 1.0, 4), dtype=dtype).astype(np.float64),
                  kappa=rng.uniform(0.2, 1.0, (4, stride)).astype(dtype), xi0=signed(), xin=signed(), acc=signed(),
                  u_base=rng.uniform(0.5, 2.0, n).astype(dtype), vn=rng.uniform(0.5, 2.0, n).astype(dtype), ur=rng.uniform(0.5, 2.0, n).astype(dtype),
                  dt=np.asarray([0.37], dtype=dtype).astype(np.float64), nlocal=_i1(n))

    def model(i):
        f = {k: _f64(a) for k, a in i.items()}
        dt = float(f["dt"][0])
        out = {}
        for tag, nr, perdof, st in RELAX_RUNS:
            bw, aw, kind = tableau(st, dt, dtype)
            itau = (1.0 / f["tau"][:nr]).astype(dtype).astype(np.float64)  # the kernel rounds 1 / tau to the field's type
            weights = f["kappa"][:nr, :n] if perdof else np.repeat(f["ks"][:nr].astype(dtype).astype(np.float64)[:, None], n, axis=1)
            ref = _numpy_stage(kind, bw, aw, aw, itau, weights, *(f[k][:nr, :n] for k in ("xi0", "xin", "acc")), f["u_base"], f["vn"])
            for name, rr in zip(("xi0", "xin", "acc"), ref[:3]):
                full, bound = f[name][:nr].copy(), np.zeros((nr, stride))  # the row padding keeps its bits
                full[:, :n] = rr
                written = name == "xi0" if kind == 2 else name in ("xin", "acc")
                if written:
                    bound[:, :n] = 16 * eps * max(1.0, float(np.max(np.abs(rr))))
                out[f"{tag}.{name}"] = Check("abs", full.reshape(-1), bound.reshape(-1))
            out[f"{tag}.ur"] = Check("abs", ref[3], np.full(n, 16 * eps * max(1.0, float(np.max(np.abs(ref[3]))))))
        return out

    states = tuple(tuple(f"{tag}.{name}" for name in ("xi0", "xin", "acc")) for tag, *_ in RELAX_RUNS)
    return [Group(name, inputs, model, [(("xi0", "xin", "acc"), states)]) for name in ("rel_a", "rel_s")]


def stage_exchanged(group, a, b):
    """``exchanged`` for the two stage groups, whose outputs are named ``<run>.<vector>``."""
    inp = dict(group.inputs)
    inp[a], inp[b] = inp[b], inp[a]
    out = dict(group.model(inp))
    for k in list(out):
        tag, _, name = k.rpartition(".")
        if name == a and f"{tag}.{b}" in out:
            out[k], out[f"{tag}.{b}"] = out[f"{tag}.{b}"], out[k]
    return out


LOOP_STEPS = 3


def loop_group(dtype):
    """Three RK4 steps of ``StiffnessSpectral3D<T, 4>`` (cell constants -k, geometry from the vertices) + ``BioheatStage`` on the
    perturbed (2, 2, 2) box against ``CpuBioheat.advance``: the case and the bar of tests/test_bioheat_gpu.py::test_solver_against_cpu_loop."""
    import test_bioheat_gpu as tb

    gll, pre = pkg("gll"), pkg("precompute")
    P, steps, cells, perturb = 4, LOOP_STEPS, (2, 2, 2), 0.15
    # the set-up of test_bioheat_gpu._reference_run; its slab of a second material needs three cells across, so here every other cell
    # is the bone-like one
    mesh64 = pkg("boxmesh").BoxMesh(P, cells, perturb=perturb, length=1.0)
    mesh = mesh64 if dtype == np.float64 else pkg("boxmesh").BoxMesh(P, cells, perturb=perturb, length=1.0, dtype=np.float32)
    odd = np.arange(mesh64.ncells) % 2 == 1
    k, rho_c = np.where(odd, 0.32, 0.5), np.where(odd, 1900.0 * 1300.0, 1050.0 * 3600.0)
    lam = bioheat_cpu.CpuBioheat(mesh64, k, rho_c).lambda_max()
    wb = np.where(odd, 0.05, 0.2) * lam * rho_c / tb.RHO_B_C_B
    dt = float(dtype(0.8 * 2.785 / (1.25 * lam)))
    q = 32.0 * rho_c.min() / (0.5 * steps * dt) * bioheat_cpu.smooth_field(mesh64, 11)
    cpu = bioheat_cpu.CpuBioheat(mesh64, k, rho_c, wb * tb.RHO_B_C_B)
    cpu.set_heat_source(q)
    gate = bioheat_cpu.gate_of((0.0, 0.5 * steps * dt))
    sb = pkg("solver_base")
    gates = np.array([[gate(t0 + sb.C_RUNGE[i] * h) for i in range(4)] for t0, h in sb.rk4_steps(0.0, steps * dt, dt, steps)])
    inputs0 = dict(negk=(-cpu.k).astype(dtype), minv=cpu.minv.astype(dtype), pr=cpu.pr.astype(dtype), s=cpu.s.astype(dtype), T=cpu.T.astype(dtype))
    cpu.advance(0.0, steps * dt, dt, power=(0.0, 0.5 * steps * dt), max_steps=steps)
    T_ref, cem_ref = cpu.T.copy(), cpu.cem43.copy()
    pts, wts, D = gll.tabulate_1d(P, dtype)
    inputs = dict(ndofs=_i1(mesh.ndofs), x_g=np.asarray(mesh.x_g, dtype=dtype), x_dofs=mesh.x_dofs, dofmap=mesh.dofmap, dphi=D,
                  dphi_p1=pre.tabulate_hex_p1_gradients(gll.tensor_points_3d(pts), dtype), w3=gll.tensor_weights_3d(wts).astype(dtype),
                  gates=gates.astype(dtype), **inputs0, scalars=np.asarray([dt, cpu.Ta], dtype=dtype).astype(np.float64))

    def check(got, i):
        tb._check_against_cpu(got["T"], got["cem43"], T_ref, cem_ref, dtype)
        return np.zeros(1), np.zeros(1)

    def peak(got, i):  # the running maximum is never below the last temperature
        return np.maximum(got["T"] - got["tmax"], 0.0), np.zeros(got["T"].size)

    return Group("loop", inputs, lambda i: dict(T=Check("own", check), tmax=Check("own", peak)), [])


def degree_groups(P, dtype):
    """The groups of one (P, type) run of the driver."""
    return [cell_group(P, dtype), colliding_group(P, dtype), probe_group(P, dtype), psource_group(P, dtype)] + ([declined_group(dtype)] if P == 1 else [])


def free_groups(dtype):
    """The groups of the degree-free functors (run at P = 4, the degree of the composed loop)."""
    return [facet_group(dtype), receive_group(dtype)] + monitor_group(dtype) + bioheat_group(dtype) + relax_group(dtype) + [loop_group(dtype)]


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def ratio(check, got, dtype):
    """The error of ``got`` over its bar (<= 1 passes): for "tol" the larger of rel l2 / TOL.l2 and rel max / TOL.mx; for "abs" the
    largest |got - ref| / bound (entries with bound 0 must be equal); for "bits" 0 or inf."""
    ref = _f64(check.ref).reshape(-1)
    got = _f64(got).reshape(-1)
    if got.shape != ref.shape:
        return float("inf")
    if check.kind == "bits":
        return 0.0 if np.array_equal(got, ref) else float("inf")
    with np.errstate(invalid="ignore"):
        err = np.where(got == ref, 0.0, np.abs(got - ref))  # (equal infinities differ by nothing)
    if check.kind == "tol":
        tol = TOL[np.dtype(dtype)]
        return max(float(np.linalg.norm(err) / max(np.linalg.norm(ref), 1e-300)) / tol["l2"], float(np.max(err) / max(np.max(np.abs(ref)), 1e-300)) / tol["mx"])
    return _over(err, _f64(check.bound).reshape(-1))


def _over(err, bound):
    if np.any((bound == 0) & (err != 0)) or np.any(np.isnan(err)):
        return float("inf")
    live = bound > 0
    return float(np.max(err[live] / bound[live])) if live.any() else 0.0


def verify(group, got, dtype, figures=None):
    """Every output of ``group`` in ``got`` (the driver's arrays) against its bar; ``figures`` collects ``{group.output: error / bar}``."""
    failed = []
    expected = group.model(group.inputs)
    for name, c in expected.items():
        if c.kind == "same":
            r = 0.0 if np.array_equal(got[name.rsplit("_same", 1)[0]] if name.endswith("_same") else got[name], got[c.ref]) else float("inf")
        elif c.kind == "own":
            r = _over(*(np.asarray(a, dtype=np.float64).reshape(-1) for a in c.ref(got, group.inputs)))
        elif name not in got:
            r = float("inf")
        else:
            r = ratio(c, got[name], dtype)
        if figures is not None:
            figures[f"{group.name}.{name}"] = r
        if not r <= 1.0:
            failed.append((name, r))
    assert not failed, f"{group.name}: error over its bar: {failed}"
