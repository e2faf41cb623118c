#!/usr/bin/env python3
"""
Linear plane wave in a box, explicit RK4, on the MI355X operators -- the counterpart of the
reference's cuda/demo_linear_box.py (same physical parameters :53-80, time-step rule :115-122,
stage sequence :487-566, final-plane sampling :128-141) on the synthetic structured mesh that
replaces dolfinx's ``create_box``.

    python fenicsx-fus-gpu_amd/demo_linear_box.py [--cells N] [--degree P] [--reference-sequence] [--out file.npz]
    python fenicsx-fus-gpu_amd/demo_linear_box.py --array 8,8 --focus 0.06,0.05,0.06     # phased array focused on a point
    python fenicsx-fus-gpu_amd/demo_linear_box.py --length 0.012 --cells 8 --time-reversal 0.011 0.0063 0.0058 --elements 3 3
                                                   # listen to a virtual source at the focus through an aberrating slab, fire back
    python fenicsx-fus-gpu_amd/demo_linear_box.py --length 0.012 --cells 8 --time-reversal 0.011 0.0063 0.0058 --elements 3 3 --pulse 3
                                                   # the same with a 3-cycle pulse: re-emit the recorded SIGNALS reversed in time
    python fenicsx-fus-gpu_amd/demo_linear_box.py --source-waveform rows.npy 2.5e-8       # drive the source with sampled rows [R, Nt]
    python fenicsx-fus-gpu_amd/demo_linear_box.py --nodal-lens                             # c and rho given at the dofs: a smooth inclusion
    python -m torch.distributed.run --nproc-per-node 8 fenicsx-fus-gpu_amd/demo_linear_box.py   # one rank per GPU

Prints the reference's progress / timing lines (cuda/demo_linear_box.py:125,183,569-581) and
optionally stores the pressure field sampled on the z = 0 plane of the dof grid.
"""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--cells", type=int, default=None, help="cells per direction of the WHOLE box, split over the ranks' blocks -- the reference's fixed-size "
                         "box, strong scaling (default: 2 per wavelength, as the reference)")
    ap.add_argument("--reference-sequence", action="store_true", help="the reference's unfused launch sequence")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--eval-out", default=None, metavar="DIR",
                    help="evaluate the final pressure field at the reference's 100 x 100 points of the z = 0 plane and append the rows "
                         "'x,y,value' to DIR/pressure_field_nproc<N>.txt, rank after rank (cuda/demo_linear_box.py:128-141,587-605)")
    ap.add_argument("--device-eval", action="store_true",
                    help="--eval-out evaluates on the device (sensors.PointSensors.evaluate) instead of the host's eval_function; same rows")
    ap.add_argument("--array", default=None, metavar="NY,NZ",
                    help="split the source face x = 0 into NY x NZ elements (sources.SourceArray) with delays that focus on --focus, and "
                         "report the peak pressure at the focus and along the x axis through it, recorded on the device every step")
    ap.add_argument("--focus", default=None, metavar="X,Y,Z", help="focal point of --array in m (default: the centre of the box)")
    ap.add_argument("--sponge", type=int, default=0, metavar="CELLS",
                    help="absorbing sponge layer of CELLS cells inside the four lateral faces (y and z), which the reference leaves rigid "
                         "(sponge.SpongeLayer: one sparse damping launch per stage); default 0: off")
    ap.add_argument("--length", type=float, default=0.12, help="edge of the box in m (default: the reference's 0.12)")
    ap.add_argument("--power-law", type=float, nargs=2, default=None, metavar=("ALPHA0", "Y"),
                    help="tissue absorption ALPHA0 f^Y (dB/cm/MHz^Y, Y in 1 .. 1.5) through two relaxation mechanisms fitted between half and "
                         "five times the source frequency (relaxation.fit_power_law, without a thermoviscous term: the linear model has "
                         "none); prints the fit's largest relative error; default: no volume loss")
    ap.add_argument("--time-reversal", type=float, nargs=3, default=None, metavar=("FX", "FY", "FZ"),
                    help="time-reversal focusing on the point (FX, FY, FZ) through an aberrating slab (twice the speed of sound, one "
                         "wavelength thick, in front of the y > L/2 half of the aperture): a receive run with a virtual point source at the "
                         "focus (sources.PointSources, receivers.ElementReceivers), then transmit runs with the conjugate phases "
                         "(receivers.time_reversal) and with the geometric ones (sources.focus_phases); prints the first-harmonic "
                         "amplitude at the focus of both.  One rank; composes with --sponge")
    ap.add_argument("--nodal-lens", action="store_true",
                    help="a nodal medium (nodal_medium.NodalMedium): c and rho given at the dofs, not per cell -- a smooth Gaussian inclusion "
                         "(c 1500 -> 1800 m/s, rho 1000 -> 1200 kg/m^3, radius L/6) at the centre of the box; the stiffness apply takes 1/rho "
                         "inside its contraction (csrc/stiffness_geom_nodal.hpp).  Composes with --sponge, --array, --power-law and ranks")
    ap.add_argument("--pulse", type=float, default=None, metavar="CYCLES",
                    help="--time-reversal with a Gaussian-modulated pulse of CYCLES cycles instead of a continuous wave: the virtual source "
                         "emits the pulse from a table (sources.SampledWaveform), the elements record every step, and the array re-emits the "
                         "recorded signals reversed in time (receivers.time_reversed_waveform); prints the refocus time and the peak at the "
                         "focus against the same pulse fired with geometric delays.  Without --pulse: the harmonic phases")
    ap.add_argument("--source-waveform", nargs=2, default=None, metavar=("FILE.npy", "DT"),
                    help="drive the source with the sampled rows of FILE.npy ([Nt] or [R, Nt], sample interval DT seconds, first sample at "
                         "t = 0, zero after the last; sources.SampledWaveform) instead of the analytic waveform: the whole source face "
                         "(R = 1) or, with --array, its elements (R = 1 or one row per element, on top of the focusing delays)")
    ap.add_argument("--energy", type=int, default=0, metavar="EVERY",
                    help="record the energy 1/2 v.Mv + 1/2 u.Ku on the device after every EVERY-th step (diagnostics.EnergyRecorder); the series "
                         "goes to <--out or linear_box>.energy.npz")
    ap.add_argument("--guard", type=int, default=0, metavar="EVERY",
                    help="check max |u| and the non-finite count every EVERY steps (diagnostics.FieldGuard): a run that goes unstable stops there")
    ap.add_argument("--stable-dt", action="store_true",
                    help="print the operator-based RK4 limit of this mesh and medium (solver.stable_time_step) beside the snapped CFL step")
    ap.add_argument("--elements", type=int, nargs=2, default=(4, 4), metavar=("NY", "NZ"), help="elements of the --time-reversal array (default 4 4)")
    a = ap.parse_args()
    if a.focus and not a.array:
        ap.error("--focus needs --array")
    if a.pulse is not None and not a.time_reversal:
        ap.error("--pulse needs --time-reversal")
    if a.pulse is not None and not a.pulse > 0.0:
        ap.error("--pulse: a positive number of cycles")
    if a.source_waveform and a.time_reversal:
        ap.error("--time-reversal builds its own sources")
    if a.time_reversal and a.nodal_lens:
        ap.error("--time-reversal builds its own (per-cell) medium")
    if a.time_reversal and (a.array or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--time-reversal runs on one rank and builds its own array (--elements)")

    import torch
    import torch.distributed as dist

    import fusgpu_loader

    boxmesh, ls, scat = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "scatterer"))
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    comm = None
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
        comm = scat.default_comm()  # exchange issued by libfusgpu.so (PEER transport; FUS_HALO=native: RCCL); torch.distributed only bootstraps it

    # cuda/demo_linear_box.py:53-80
    float_type = np.float64
    source_frequency, source_amplitude = 0.5e6, 60000.0
    speed_of_sound, density = 1500.0, 1000.0
    domain_length = a.length
    wave_length = speed_of_sound / source_frequency
    num_element = a.cells if a.cells is not None else int(2 * domain_length / wave_length)
    grid = boxmesh.default_grid(world)
    mesh = boxmesh.BoxMesh(a.degree, num_element, grid=grid, rank=rank, length=domain_length, dtype=float_type)
    medium = None
    if a.nodal_lens:
        # callables of position: every rank evaluates them at its own dofs, ghosts included, so the values agree across ranks
        centre, r2 = 0.5 * np.asarray(mesh.length), (domain_length / 6.0) ** 2
        bump = lambda xyz: np.exp(-np.sum((xyz - centre) ** 2, axis=1) / r2)  # noqa: E731
        medium = fusgpu_loader.submodule("nodal_medium").NodalMedium(lambda xyz: speed_of_sound + 300.0 * bump(xyz),
                                                                     lambda xyz: density + 200.0 * bump(xyz))
    # (the time-step rule takes the fastest speed of the medium)
    h = ls.time_step_parameters(mesh, a.degree, speed_of_sound, source_frequency, domain_length)
    if world > 1:
        hm = torch.tensor([h], dtype=torch.float64, device="cuda")
        dist.all_reduce(hm, op=dist.ReduceOp.MIN)  # comm.Allreduce(hmin, mesh_size, op=MPI.MIN), :108
        h = float(hm.item())
    dt, tf, nstep = ls.snap_time_step(h, a.degree, speed_of_sound + (300.0 if a.nodal_lens else 0.0), source_frequency, domain_length)
    if rank == 0:
        print(f"Number of steps: {nstep}", flush=True)
        print(f"Number of degrees-of-freedom: {mesh.ndofs_global}", flush=True)
    source, probes = None, None
    if a.array:
        src, sens = fusgpu_loader.submodule("sources"), fusgpu_loader.submodule("sensors")
        ny, nz = (int(v) for v in a.array.split(","))
        L = domain_length
        focus = np.array([float(v) for v in a.focus.split(",")] if a.focus else [0.5 * L] * 3)
        centres = src.grid_centres(ny, nz, 0.0, (0.0, L), (0.0, L))  # the global layout: every rank assigns its facets by centroid
        source = src.SourceArray(src.grid_elements(ny, nz, (0.0, L), (0.0, L)), delay=src.focus_delays(centres, focus, speed_of_sound),
                                 n_elements=ny * nz)
        # the focus and 64 points along the x axis through it: running peaks on the device (sensors.PointSensors)
        axis = np.stack([np.linspace(0.0, L, 64), np.full(64, focus[1]), np.full(64, focus[2])], axis=1)
        pts = np.concatenate([focus[None, :], axis])
        probes = (pts, sens.PointSensors(mesh, pts, float_type, peak=True))
    if a.source_waveform:
        src = fusgpu_loader.submodule("sources")
        try:
            wf = src.SampledWaveform(np.load(a.source_waveform[0]), float(a.source_waveform[1]))
            if source is None:  # the scalar source: one element that holds every source facet
                source = src.SourceArray(lambda cen: np.zeros(len(cen), dtype=np.int64), n_elements=1, waveform=wf)
            else:
                source = src.SourceArray(source.element_of_facet, delay=source.delay, n_elements=source.n_elements, waveform=wf)
        except (OSError, ValueError) as e:
            raise SystemExit(f"--source-waveform: {e}") from None
        if rank == 0:
            print(f"Source waveform: {wf.n_rows} row(s) of {wf.n_samples} samples every {wf.dt:g} s (until t = {wf.t_end:g} s)", flush=True)
    sponge = None
    if a.sponge:
        sp = fusgpu_loader.submodule("sponge")
        if not 0 < a.sponge <= num_element // 2:
            raise SystemExit(f"--sponge: 1 .. {num_element // 2} cells")
        # the GLOBAL box, so every rank evaluates the same profile on its own dofs
        sponge = sp.SpongeLayer(sp.box_profile((0.0, 0.0, 0.0), mesh.length, a.sponge * domain_length / num_element, sp.LATERAL, speed_of_sound))
    relaxation = None
    if a.power_law:
        rx = fusgpu_loader.submodule("relaxation")
        fit = rx.fit_power_law(a.power_law[0], a.power_law[1], 0.5 * source_frequency, 5.0 * source_frequency, n=2,
                               speed_of_sound=speed_of_sound, with_thermoviscous=False)
        relaxation = rx.RelaxationAbsorption(fit.tau, fit.kappa)
        try:
            relaxation.check_time_step(dt)  # a coarse mesh (few --cells) steps past the fastest mechanism
        except ValueError as e:
            raise SystemExit(f"--power-law: {e}") from None
        if rank == 0:
            print(f"Power law {a.power_law[0]:g} dB/cm/MHz^{a.power_law[1]:g}: tau = {fit.tau}, kappa = {fit.kappa}, largest relative error of "
                  f"the fit {fit.max_rel_error:.4f}; alpha_r(f0) = {relaxation.alpha(source_frequency, speed_of_sound):.4g} Np/m", flush=True)
    if a.time_reversal:
        if relaxation is not None:
            raise SystemExit("--power-law does not compose with --time-reversal")
        return time_reversal_run(a, mesh, sponge, float_type, speed_of_sound, density, source_frequency, source_amplitude)
    solver = ls.LinearSpectral3D(mesh, float_type, speed_of_sound, density, source_frequency, source_amplitude,
                                 comm=comm, fused=not a.reference_sequence, source=source, sponge=sponge, relaxation=relaxation,
                                 nodal_medium=medium)
    solver.init()
    if medium is not None and rank == 0:
        print(f"Nodal medium: c {solver.c_nodal.min():.1f} .. {solver.c_nodal.max():.1f} m/s, rho {solver.rho_nodal.min():.1f} .. "
              f"{solver.rho_nodal.max():.1f} kg/m^3 at the dofs; reference speed of the source {solver.c0:.1f} m/s", flush=True)
    if sponge is not None:
        n_layer = solver._sponge[0].numel()
        print(f"Sponge layer (rank {rank}): {a.sponge} cell(s) wide, {n_layer} owned dofs, sigma_max dt = {sponge.sigma_max * dt:.3f}", flush=True)
    if a.stable_dt:
        dt_op = solver.stable_time_step(0.8)
        if rank == 0:
            print(f"Stable step from the operators: {dt_op:.6e} s at safety 0.8 (limit {solver.stable_limit:.6e} s: lambda_max "
                  f"{solver.lambda_max:.4e}, damping_max {solver.damping_max:.4e}); snapped CFL step: {dt:.6e} s", flush=True)
    diag = fusgpu_loader.submodule("diagnostics")
    energy = diag.EnergyRecorder(solver, every=a.energy, capacity=nstep // a.energy + 1) if a.energy else None
    guard = diag.FieldGuard(every=a.guard) if a.guard else None
    if rank == 0:
        print("Solve!", flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t, steps = solver.rk4(0.0, tf, dt, max_steps=a.max_steps, sensors=probes[1] if probes else None, energy=energy, guard=guard)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if rank == 0:
        print(f"t: {t:5.5},\t Steps: {steps}/{nstep}", flush=True)
        print(f"Solve time: {el}")
        print(f"Solve time per step: {el / max(steps, 1)}")
    if energy is not None:
        te, kin, pot, tot, amax, bad = energy.energies()
        if rank == 0 and len(te):
            name = f"{a.out or 'linear_box'}.energy.npz"
            np.savez(name, t=te, kinetic=kin, potential=pot, total=tot, absmax=amax, nonfinite=bad)
            print(f"Energy: {len(te)} records, first {tot[0]:.6e} (t = {te[0]:.4e}), last {tot[-1]:.6e} (t = {te[-1]:.4e}) -> {name}", flush=True)
    if probes is not None:
        pts, s = probes
        pmax = s.peak()[0][None, :]
        peak = (s.gather(comm, pmax) if world > 1 else fusgpu_loader.submodule("sensors").merge([(s.point_ids, pmax)], pts.shape[0]))[0]
        if rank == 0:
            k = int(np.nanargmax(peak[1:])) + 1
            print(f"Array elements: {a.array.replace(',', ' x ')}, focus: {tuple(float(v) for v in pts[0])}")
            print(f"Peak pressure at the focus: {peak[0]}")
            print(f"Peak pressure on the axis: {peak[k]} at x = {pts[k, 0]}")
    if a.out:
        lex = mesh.global_lexicographic_ids()[: mesh.nlocal]
        gd = mesh.global_dof_dims
        on_plane = (lex % gd[2]) == 0  # z = 0 plane of the dof grid
        np.savez(a.out if world == 1 else f"{a.out}.rank{rank}", lex=lex[on_plane], u=solver.u_sol()[on_plane],
                 dims=np.array(gd), t=t, steps=steps)
    if a.eval_out:
        pe = fusgpu_loader.submodule("point_evaluation")
        xp = np.linspace(0, domain_length, 100, dtype=float_type)  # :130-139
        X_p, Y_p = np.meshgrid(xp, xp)
        points = np.zeros((3, 100 * 100), dtype=float_type)
        points[0], points[1] = X_p.flatten(), Y_p.flatten()
        if a.device_eval:
            sens = fusgpu_loader.submodule("sensors").PointSensors(mesh, points, float_type)
            if solver.halo is not None:
                solver.halo.fwd(solver.u)  # the ghosts the points' cells read
            order = np.argsort(sens.point_ids)  # the caller's point order, as compute_eval_params keeps it
            data = np.zeros((order.size, 3))
            data[:, 0], data[:, 1] = sens.points[order, 0], sens.points[order, 1]
            data[:, 2] = sens.evaluate(solver.u).cpu().numpy()[order]
        else:
            x_eval, cell_eval = pe.compute_eval_params(mesh, points, float_type)
            u_full = solver.u_sol(with_ghosts=True)
            data = np.zeros_like(x_eval)
            if len(cell_eval):
                data[:, 0], data[:, 1] = x_eval[:, 0], x_eval[:, 1]
                data[:, 2] = pe.eval_function(mesh, u_full, x_eval, cell_eval)
        if rank == 0:
            os.makedirs(a.eval_out, exist_ok=True)
        for i in range(world):  # :597-605: one rank after the other appends to the same file
            if world > 1:
                dist.barrier()
            if rank == i:
                with open(os.path.join(a.eval_out, f"pressure_field_nproc{world}.txt"), "a") as f:
                    np.savetxt(f, data, fmt="%.8f", delimiter=",")
    if world > 1:
        dist.destroy_process_group()


def time_reversal_run(a, mesh, sponge, float_type, c0, density, f0, p0):
    """--time-reversal: listen to a virtual point source at the focus through the slab, then fire the array with the conjugate and
    with the geometric phases and compare the first harmonic at the focus (recorded on the device over the last two periods)."""
    import fusgpu_loader

    ls, src, rxm, sens = (fusgpu_loader.submodule(m) for m in ("linear_solver", "sources", "receivers", "sensors"))
    L, lam, period = mesh.length, c0 / f0, 1.0 / f0
    focus = np.asarray(a.time_reversal, dtype=np.float64)[None, :]
    ny, nz = a.elements
    cen = mesh.x_g.astype(np.float64)[mesh.x_dofs].mean(axis=1)
    slab = (cen[:, 0] > lam) & (cen[:, 0] < 2.0 * lam) & (cen[:, 1] > 0.5 * L[1])
    if not slab.any() or np.any(np.abs(cen[slab] - focus).max(axis=1) < 0.5 * mesh.h[0]):
        raise SystemExit("--time-reversal: the slab (x in (lambda, 2 lambda), y > L/2) holds no cell of this mesh, or the focus lies in it")
    c = np.where(slab, 2.0 * c0, c0)
    dt, _, _ = ls.snap_time_step(ls.time_step_parameters(mesh, a.degree, 2.0 * c0, f0, L[0]), a.degree, 2.0 * c0, f0, L[0])
    tf = L[0] / c0 + 8.0 * period  # the ramp (4 periods), the transit, and the two periods that are recorded
    kw = dict(speed_of_sound=c, density=density, source_frequency=f0, reference_speed_of_sound=c0, fused=not a.reference_sequence, sponge=sponge)
    grid = src.grid_elements(ny, nz, (0.0, L[1]), (0.0, L[2]))
    print(f"Time reversal: focus {tuple(float(v) for v in focus[0])}, {ny} x {nz} elements, slab of {int(slab.sum())} cells at c = {2.0 * c0}, "
          f"{int(round(tf / dt))} steps per run", flush=True)
    if a.pulse is not None:
        return pulse_reversal_run(a, mesh, kw, grid, focus, float_type, c0, f0, p0, dt)
    listen = ls.LinearSpectral3D(mesh, float_type, source_amplitude=0.0, point_source=src.PointSources(focus), **kw)
    rx = rxm.ElementReceivers(mesh, grid, float_type, harmonics=(1,), frequency=f0, n_elements=ny * nz, detJ=listen.detJ_f1)
    listen.init()
    listen.rk4(0.0, tf, dt, max_steps=a.max_steps, receivers=rx, record_from=tf - 2.0 * period)
    R = rx.harmonic(1)

    def transmit(array):
        s = ls.LinearSpectral3D(mesh, float_type, source_amplitude=p0, source=array, **kw)
        probe = sens.PointSensors(mesh, focus, float_type, harmonics=(1,), frequency=f0)
        s.init()
        s.rk4(0.0, tf, dt, max_steps=a.max_steps, sensors=probe, record_from=tf - 2.0 * period)
        return float(probe.harmonic_amplitude(1)[0]), s

    a_tr, s = transmit(rxm.time_reversal(rx))
    centres = src.grid_centres(ny, nz, 0.0, (0.0, L[1]), (0.0, L[2]))
    a_geo, _ = transmit(src.SourceArray(grid, phase=src.focus_phases(centres, focus[0], c0, f0), n_elements=ny * nz))
    bound = s.p0 * s.w0 / s.c0 / density * float(np.sum(rx.areas() * np.abs(R)))  # reciprocity: sum_e |G_e|
    print(f"First-harmonic amplitude at the focus: time reversal {a_tr:.6g}, geometric (focus_phases) {a_geo:.6g}")
    print(f"Time-reversal gain over the geometric phases: {a_tr / a_geo:.3f} ({a_tr / bound:.3f} of the reciprocity bound {bound:.6g})")


def pulse_reversal_run(a, mesh, kw, grid, focus, float_type, c0, f0, p0, dt):
    """--time-reversal --pulse: the listen, reverse and transmit chain with the signals themselves.  The virtual source emits
    exp(-((t - t_c) / sigma)^2 / 2) cos(w0 (t - t_c)), 4 sigma = CYCLES periods, from a table; every element records every step; the
    array re-emits row e reversed in time, and the pressure at the focus peaks at T_run - t_c."""
    import fusgpu_loader

    ls, src, rxm, sens = (fusgpu_loader.submodule(m) for m in ("linear_solver", "sources", "receivers", "sensors"))
    L, period = mesh.length, 1.0 / f0
    ny, nz = a.elements
    sigma = 0.25 * a.pulse * period
    t_c = 4.0 * sigma
    nsteps = int(np.ceil((2.0 * t_c + 1.5 * L[0] / c0 + 2.0 * period) / dt))  # the pulse, the transit with room for the slab's echoes
    if a.max_steps is not None:
        nsteps = min(nsteps, a.max_steps)
    t_run = nsteps * dt
    t = np.arange(nsteps + 2) * dt
    pulse = src.SampledWaveform(np.exp(-0.5 * ((t - t_c) / sigma) ** 2) * np.cos(2.0 * np.pi * f0 * (t - t_c)), dt)
    listen = ls.LinearSpectral3D(mesh, float_type, source_amplitude=0.0, point_source=src.PointSources(focus, waveform=pulse), **kw)
    rx = rxm.ElementReceivers(mesh, grid, float_type, capacity=nsteps, n_elements=ny * nz, detJ=listen.detJ_f1)
    listen.init()
    listen.rk4(0.0, t_run + dt, dt, max_steps=nsteps, receivers=rx)

    def transmit(array):
        s = ls.LinearSpectral3D(mesh, float_type, source_amplitude=p0, source=array, **kw)
        probe = sens.PointSensors(mesh, focus, float_type, capacity=nsteps)
        s.init()
        s.rk4(0.0, t_run + dt, dt, max_steps=nsteps, sensors=probe)
        p = np.abs(probe.series()[:, 0])
        k = int(np.argmax(p))
        return float(p[k]), (k + 1) * dt

    p_tr, t_tr = transmit(rxm.time_reversed_waveform(rx, dt, taper=0.05))
    centres = src.grid_centres(ny, nz, 0.0, (0.0, L[1]), (0.0, L[2]))
    p_geo, _ = transmit(src.SourceArray(grid, delay=src.focus_delays(centres, focus[0], c0), n_elements=ny * nz, waveform=pulse))
    print(f"Pulse of {a.pulse:g} cycles centred at t_c = {t_c:.6g} s; {nsteps} steps per run, T_run = {t_run:.6g} s")
    print(f"Refocus time: {t_tr:.6g} s (expected T_run - t_c = {t_run - t_c:.6g} s, {abs(t_tr - (t_run - t_c)) / period:.3f} periods off)")
    print(f"Peak |p| at the focus: time-reversed signals {p_tr:.6g}, geometric delays (focus_delays) {p_geo:.6g}, ratio {p_tr / p_geo:.3f}")


if __name__ == "__main__":
    main()
