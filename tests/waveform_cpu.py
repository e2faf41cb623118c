"""Host model of sources that carry a sampled waveform (test infrastructure): the signals the tests drive them with, a numpy
restatement of the facet launch of csrc/source_wave.hpp, and the array source as a ``source_term`` hook of
``oracle.rk4_oracle.solve`` / ``solve_westervelt``.  Everything goes through ``SourceArray.values`` / ``PointSources.values``, i.e.
``SampledWaveform.values``; the point sources' hook is ``point_source_cpu.point_term``, unchanged."""

import numpy as np

from conftest import pkg
from oracle import oracle_np


def gaussian_pulse(t, f0, t_c, cycles=1.0):
    """``exp(-((t - t_c) / (cycles T))^2 / 2) cos(w0 (t - t_c))`` and its time derivative: a pulse no analytic source represents."""
    T, w0 = 1.0 / f0, 2.0 * np.pi * f0
    s = np.asarray(t, dtype=np.float64) - t_c
    sig = cycles * T
    env = np.exp(-0.5 * (s / sig) ** 2)
    return env * np.cos(w0 * s), env * (-(s / sig**2) * np.cos(w0 * s) - w0 * np.sin(w0 * s))


def pulse_waveform(f0, dt, nt, t_c, cycles=1.0, rows=1):
    """A ``SampledWaveform`` of ``rows`` Gaussian pulses (row r: centre ``t_c + 0.3 r T``, sign alternating), ``nt`` samples every
    ``dt`` from 0, with the stencil derivative."""
    t = np.arange(nt) * dt
    w = np.stack([(-1.0) ** r * gaussian_pulse(t, f0, t_c + 0.3 * r / f0, cycles)[0] for r in range(rows)])
    return pkg("sources").SampledWaveform(w, dt)


def analytic_table(array, frequency, dt, nt):
    """The analytic waveform of the elements of ``array`` (a ``SourceArray`` without waveform: its phases and burst, NOT its amplitudes
    and delays, which stay per-element parameters) sampled every ``dt`` with the analytic derivative: a ``SampledWaveform`` of E rows."""
    src = pkg("sources")
    E = array.n_elements
    t = np.arange(nt) * dt
    gd = [src._waveform(tk, frequency, 1.0, np.ones(E), array.phase, np.zeros(E), array.duration) for tk in t]
    return src.SampledWaveform(np.array([g for g, _ in gd]).T, dt, derivative=np.array([d for _, d in gd]).T)


def facet_reference(ndofs, g, dg, ids, c1, c2, detJ, dofmap, field=None):
    """y of one facet launch in fp64: set A with the element values ``(g, dg)`` [E] of the facets' elements ``ids`` (-1: inactive),
    ``c2`` None for the linear solver, and set B ``field = (x, c, detJ, dofmap)``."""
    act = ids >= 0
    e = np.where(act, ids, 0)
    val = np.where(act, g[e] * c1.astype(np.float64) + (dg[e] * c2.astype(np.float64) if c2 is not None else 0.0), 0.0)
    y = np.zeros(ndofs)
    oracle_np.mass_apply(np.ones(ndofs), val, y, detJ.astype(np.float64), dofmap)
    if field is not None:
        x, c, dB, dmB = field
        oracle_np.mass_apply(x.astype(np.float64), c.astype(np.float64), y, dB.astype(np.float64), dmB)
    return y


def array_term(mesh, array, f0, scale):
    """``source_term(t, b, coefficients, detJ, dofmap)`` of the array source: per facet its element's ``(g, dg)`` at the stage's source
    time, ``g`` against the first coefficient and -- Westervelt -- ``dg`` against the second."""
    ids = array.assign(mesh, mesh.boundary_facets([2]))
    act = ids >= 0
    e = np.where(act, ids, 0)

    def term(t, b, coefficients, detJ, dofmap):
        g, dg = array.values(t, f0, scale)
        val = np.where(act, g[e], 0.0) * coefficients[0]
        if len(coefficients) > 1:
            val = val + np.where(act, dg[e], 0.0) * coefficients[1]
        np.add.at(b, dofmap, val[:, None] * detJ)

    return term


# ---- time reversal of the signals through the aberrating slab: the case and its CPU model -------------------------------------------------
def slab_case(thickness_cells=2):
    """The slab case of tests/test_receivers_gpu.py::test_time_reversal_focuses_through_an_aberrating_slab (P = 4, 8 x 6 x 6 cells of
    1.5 mm, f0 = 0.5 MHz, c = 1500 with a slab c = 3000 over the cells with x-centroid in (2h, (2 + thickness) h) and y-centroid >
    Ly / 2, a 3 x 3 array, the focus (7.3h, Ly/2 + 0.2h, Lz/2 - 0.1h), dt from c = 3000) with a PULSE instead of a continuous wave:
    exp(-((t - 4T) / T)^2 / 2) cos(w0 (t - 4T)), a run of 14 periods, sampled every step."""
    boxmesh, ls, src = pkg("boxmesh"), pkg("linear_solver"), pkg("sources")
    f0, P, cells, h = 0.5e6, 4, (8, 6, 6), 1.5e-3
    T = 1.0 / f0
    L = tuple(h * n for n in cells)
    mesh = boxmesh.BoxMesh(P, cells, length=L)
    cen = mesh.x_g.astype(np.float64)[mesh.x_dofs].mean(axis=1)
    c = np.where((cen[:, 0] > 2 * h) & (cen[:, 0] < (2 + thickness_cells) * h) & (cen[:, 1] > L[1] / 2), 3000.0, 1500.0)
    dt, _, _ = ls.snap_time_step(ls.time_step_parameters(mesh, P, 3000.0, f0, L[0]), P, 3000.0, f0, L[0])
    nsteps = int(round(14 * T / dt))
    t_c = 4 * T
    pulse = src.SampledWaveform(gaussian_pulse(np.arange(nsteps + 2) * dt, f0, t_c)[0], dt)
    fn = src.grid_elements(3, 3, (0.0, L[1]), (0.0, L[2]))
    centres = src.grid_centres(3, 3, 0.0, (0.0, L[1]), (0.0, L[2]))
    focus = np.array([[7.3 * h, L[1] / 2 + 0.2 * h, L[2] / 2 - 0.1 * h]])
    return dict(mesh=mesh, c=c, rho=1000.0, f0=f0, dt=dt, nsteps=nsteps, t_c=t_c, pulse=pulse, fn=fn, centres=centres, focus=focus, L=L)


def slab_model(case, oracle_c):
    """The listen, reverse and transmit chain of ``slab_case`` on the host (oracle.rk4_oracle.solve with the source hooks above, the
    receivers of point_source_cpu.receive, the sensor as the point's Lagrange rows): ``(peak, time of the peak)`` of |p| at the focus
    for the time-reversed signals and for the same pulse fired with ``focus_delays`` computed in water."""
    import point_source_cpu
    from oracle import rk4_oracle

    src, rxm, sensors = pkg("sources"), pkg("receivers"), pkg("sensors")
    mesh, dt, nsteps, f0 = case["mesh"], case["dt"], case["nsteps"], case["f0"]
    bd = mesh.boundary_facets([2])
    ids = src.SourceArray(case["fn"], n_elements=9).assign(mesh, bd)
    fdm = np.asarray(mesh.facet_dofmap(bd)).reshape(bd.shape[0], -1)
    fdet = rk4_oracle.host_facet_detJ(mesh, bd)
    su = sensors.sensor_setup(mesh, case["focus"])
    lx, ly, lz = su.weights[0]
    wp = (lx[:, None, None] * ly[None, :, None] * lz[None, None, :]).reshape(-1)
    prow = su.rows[su.cell_index[0]]

    def run(source_term, observe):
        """``observe(u)`` of the state after every step, [nsteps, ...]: the stage hook sees the state at the start of a step at every
        fourth call (the first stage of RK4 has no increment), the last state is the loop's result."""
        seen, calls = [], [0]

        def stage_term(m):
            def term(b, un, vn):
                if calls[0] % 4 == 0 and calls[0] > 0:
                    seen.append(observe(un))
                calls[0] += 1
            return term

        u, _ = rk4_oracle.solve(mesh, nsteps, dt, c0=case["c"], rho0=case["rho"], f0=f0, c_ref=1500.0, oracle_c=oracle_c,
                                source_term=source_term, stage_term=stage_term)
        seen.append(observe(u))
        return np.array(seen)

    def heard(u):
        S, A = point_source_cpu.receive(u, ids, fdm, fdet, 9)
        return S / A

    listen = src.PointSources(case["focus"], waveform=case["pulse"])
    series = run(point_source_cpu.point_term(mesh, listen, f0), heard)
    assert series.shape == (nsteps, 9)
    A = 60000.0 * 2 * np.pi * f0 / 1500.0
    out = []
    for arr in (rxm.time_reversed_waveform(series, dt, element_of_facet=case["fn"]),
                src.SourceArray(case["fn"], delay=src.focus_delays(case["centres"], case["focus"][0], 1500.0), n_elements=9,
                                waveform=case["pulse"])):
        p = np.abs(run(array_term(mesh, arr, f0, A), lambda u: float(wp @ u[prow])))
        k = int(np.argmax(p))
        out.append((float(p[k]), (k + 1) * dt))
    return out


if __name__ == "__main__":  # python tests/waveform_cpu.py [thickness in cells]: the figures quoted in tests/test_waveform_sources_gpu.py
    import sys
    import time

    from oracle.oracle_c import OracleLib

    t0 = time.perf_counter()
    case = slab_case(int(sys.argv[1]) if len(sys.argv) > 1 else 2)
    (p_tr, t_tr), (p_geo, t_geo) = slab_model(case, OracleLib())
    T = 1.0 / case["f0"]
    print(f"{case['nsteps']} steps of {case['dt']:.6e} s; T_run - t_c = {(case['nsteps'] * case['dt'] - case['t_c']) / T:.4f} T")
    print(f"time-reversed signals: peak {p_tr:.6e} at {t_tr / T:.4f} T; geometric delays: peak {p_geo:.6e} at {t_geo / T:.4f} T; "
          f"ratio {p_tr / p_geo:.4f}  ({time.perf_counter() - t0:.0f} s)")
