#!/usr/bin/env python3
"""
Westervelt (nonlinear, attenuating) wave from a source face into a curved "bowl" geometry, explicit RK4, on the MI355X
operators -- the counterpart of the reference's cuda/demo_nonlinear_bowl.py: same physical parameters (:56-75), time-step
rule (CFL = 0.40, :119-125; final time L/c + 8/f), material coefficients (:357-374), stage sequence (:540-650: lumped
mass with the nonlinear term, two stiffness applies, mass of v_n^2, g and dg/dt source terms, absorbing facets) and the
collection of the pressure field over the LAST PERIOD (:662-680: once t > L/c + 6/f, one dump per time step for one
period), on a synthetic mesh: the reference reads the H131 transducer mesh from XDMF (absent from its repository); here
a structured box is warped by a smooth bowl map, which gives what its geometry gives the kernels -- trilinear, NON-affine
cells (G varies per quadrature point; P1 geometry, cuda/demo_nonlinear_bowl.py:317).

    python fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py [--degree 6] [--cells N] [--out-dir DIR] [--max-steps K]
    python fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py --sensor-plane 141,241 --out-dir DIR [--peak-out FILE]   # recorded on the device
    python fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py --sensor-plane 61,61 --peak-out FILE --array 6,6 --focus 0.008,0.006,0.006
    python fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py --field-stats maps.npz     # last-period maps of every dof, accumulated on the device
    python fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py --intensity                # the focus of the intensity |I| and the peak radiation force density |F|
    python fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py --nodal-lens               # c, rho, beta and alpha given at the dofs: a smooth inclusion
    python fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py --shock-capture            # a per-cell sensor adds diffusivity where the wave steepens
    python fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py --thermal 10 20            # then heat for 10 s and cool for 20 s with the last period's q (bioheat.py)
    python -m torch.distributed.run --nproc-per-node 8 fenicsx-fus-gpu_amd/demo_nonlinear_bowl.py

Dumps: ``DIR/pressure_field_<k>.txt`` for k = 0 .. steps_per_period-1, rows ``x,y,p`` on the mid-z plane of the dof grid
(the reference evaluates ``u_n.eval`` at its own point set and writes x, y, value rows with the same format string);
with several ranks every rank appends its owned points, as the reference's ranks append theirs.
"""

import argparse
import functools
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=6)
    ap.add_argument("--cells", type=int, default=None, help="cells per direction of the whole box (default: 2 per wavelength at P = 6 scale)")
    ap.add_argument("--length", type=float, default=None, help="domain length in m (reference: 0.08; default here 0.012 so the default run takes seconds)")
    ap.add_argument("--reference-sequence", action="store_true", help="the reference's unfused launch sequence (four cell kernels per stage)")
    ap.add_argument("--geometry", default="auto", choices=["auto", "kernel", "array"],
                    help="auto: G formed in the cell kernel from the vertices for the fused stage of degree >= 3 (the solver's default); "
                         "array: the reference's precomputed G array; kernel: force the kernel form")
    ap.add_argument("--in-kernel-geometry", action="store_true", help="same as --geometry kernel")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--out-dir", default=None, help="write the last-period pressure fields there")
    ap.add_argument("--sensor-plane", default=None, metavar="NX,NY",
                    help="evaluate on the device at an NX x NY grid of points on the mid-z plane of the domain (the counterpart of the "
                         "reference's own point grid, cuda/demo_linear_piston.py) and record the last period in ONE rk4 call")
    ap.add_argument("--peak-out", default=None, metavar="FILE",
                    help="with --sensor-plane: write rows 'x,y,max,min,|H1|,|H2|' over the last period to FILE")
    ap.add_argument("--array", default=None, metavar="NY,NZ",
                    help="with --sensor-plane: split the source face into NY x NZ elements (sources.SourceArray) with delays that focus on --focus")
    ap.add_argument("--focus", default=None, metavar="X,Y,Z", help="focal point of --array in m (default: the centre of the box)")
    ap.add_argument("--field-stats", default=None, metavar="FILE.npz",
                    help="accumulate the last period of EVERY owned dof on the device in ONE rk4 call (field_monitor.FieldMonitor) and "
                         "write pmax, pmin, |H1|, |H2|, the heat deposition q and the focus of |H1| to FILE.npz (several ranks: "
                         "FILE.rank<r>.npz each, the focus reduced over the ranks)")
    ap.add_argument("--intensity", action="store_true",
                    help="implies --field-stats (without a FILE.npz nothing is written): after the run, print the focus of the time-averaged intensity |I| "
                         "(intensity.py: from the harmonic maps and the gradient operator), the focal plane-wave estimate p1^2 / (2 rho c) beside it, "
                         "and the peak radiation force density |F|")
    ap.add_argument("--thermal", default=None, nargs="+", type=float, metavar=("SECONDS_ON", "SECONDS_OFF"),
                    help="implies --field-stats (without a FILE.npz nothing is written): after the acoustic run, heat soft tissue for SECONDS_ON "
                         "with the heat deposition q of the last period and cool it for SECONDS_OFF (bioheat.BioheatSpectral3D: Pennes' equation, "
                         "CEM43 thermal dose); prints the peak temperature, the focus of the dose and the volume above 240 CEM43")
    ap.add_argument("--sponge", type=int, default=0, metavar="CELLS",
                    help="absorbing sponge layer of CELLS cells inside the four lateral faces (y and z), which the reference leaves rigid "
                         "(sponge.SpongeLayer: one sparse damping launch per stage); default 0: off")
    ap.add_argument("--power-law", type=float, nargs=2, default=None, metavar=("ALPHA0", "Y"),
                    help="tissue absorption ALPHA0 f^Y (dB/cm/MHz^Y, Y in 1 .. 1.5) in place of the f^2 law of the reference's "
                         "attenuation coefficient: two relaxation mechanisms and the thermoviscous diffusivity fitted together between half "
                         "and five times the source frequency (relaxation.fit_power_law); prints the fit's largest relative error; the "
                         "heat deposition of --field-stats / --thermal is then relaxation.heat_deposition")
    ap.add_argument("--nodal-lens", action="store_true",
                    help="a nodal medium (nodal_medium.NodalMedium): c, rho, beta and alpha given at the dofs, not per cell -- a smooth Gaussian "
                         "inclusion (c 1480 -> 1780 m/s, rho 1000 -> 1200 kg/m^3, beta 3.5 -> 5, alpha 0.2 -> 5 dB/m, radius L/6) at the centre "
                         "of the box; the cell pass takes 1/rho and delta/(rho c^2) inside its two contractions "
                         "(csrc/westervelt_geom_nodal.hpp).  Composes with --sponge, --array, --field-stats, --intensity, --thermal and ranks")
    ap.add_argument("--energy", type=int, default=0, metavar="EVERY",
                    help="record the energy of the linear part, 1/2 v.M0 v + 1/2 u.Ku, on the device after every EVERY-th step "
                         "(diagnostics.EnergyRecorder); the series goes to <--out-dir or .>/energy.npz")
    ap.add_argument("--guard", type=int, default=0, metavar="EVERY",
                    help="check max |u| and the non-finite count every EVERY steps (diagnostics.FieldGuard): a run that goes unstable stops there")
    ap.add_argument("--stable-dt", action="store_true",
                    help="print the operator-based RK4 limit of this mesh and medium (solver.stable_time_step) beside the snapped CFL step")
    ap.add_argument("--source-waveform", nargs=2, default=None, metavar=("FILE.npy", "DT"),
                    help="drive the source with the sampled rows of FILE.npy ([Nt] or [R, Nt], sample interval DT seconds, first sample at "
                         "t = 0, zero after the last; sources.SampledWaveform) instead of the analytic waveform: the whole bowl (R = 1) or, "
                         "with --array, its elements (R = 1 or one row per element, on top of the focusing delays).  The interpolant's "
                         "derivative is the dg/dt of the Westervelt source term")
    ap.add_argument("--shock-capture", nargs="?", type=float, const=-1.0, default=None, metavar="STRENGTH",
                    help="shock capturing (shock_capture.ShockCapture): after every step a per-cell smoothness sensor adds up to "
                         "STRENGTH c h / P^2 of artificial diffusivity to the cells where the wave steepens (default strength: the "
                         "attachment's); prints the number of active cells and the largest diffusivity at the end.  Composes with "
                         "--stable-dt (the bound then covers the largest diffusivity), --guard and --sponge; not with --nodal-lens")
    a = ap.parse_args()
    if a.shock_capture is not None and a.nodal_lens:
        ap.error("--shock-capture: shock capturing for nodal media is out of scope (not with --nodal-lens)")
    if a.nodal_lens and (a.power_law or a.geometry == "array"):
        ap.error("--nodal-lens: the nodal cell pass forms G in the kernel (not --geometry array), and --power-law fits its own attenuation")
    if a.thermal is not None and (len(a.thermal) > 2 or min(a.thermal) < 0.0):
        ap.error("--thermal SECONDS_ON [SECONDS_OFF], both >= 0")
    if (a.field_stats or a.thermal or a.intensity) and a.sensor_plane:
        ap.error("--field-stats and --sensor-plane are separate runs")
    if a.array and not a.sensor_plane:
        ap.error("--array needs --sensor-plane")
    if a.focus and not a.array:
        ap.error("--focus needs --array")
    if a.peak_out and not a.sensor_plane:
        ap.error("--peak-out needs --sensor-plane")

    import torch
    import torch.distributed as dist

    import fusgpu_loader

    boxmesh, ls, nls, scat = (fusgpu_loader.submodule(m) for m in ("boxmesh", "linear_solver", "nonlinear_solver", "scatterer"))
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    comm = None
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
        comm = scat.default_comm()

    # cuda/demo_nonlinear_bowl.py:56-75
    float_type = np.float64
    speed_of_sound, density = 1480.0, 1000.0
    source_frequency = 1.1e6
    source_velocity = 0.38557513826589934
    source_amplitude = density * speed_of_sound * source_velocity
    period = 1.0 / source_frequency
    nonlinear_coefficient, attenuation_coefficient_dB = 3.5, 0.2
    domain_length = a.length if a.length is not None else 0.012
    wave_length = speed_of_sound / source_frequency
    P = a.degree
    num_element = a.cells if a.cells is not None else max(2, int(2 * domain_length / wave_length))
    grid = boxmesh.default_grid(world)
    L = domain_length

    def bowl(xg):  # smooth map of the box: the source face x = 0 becomes a shallow bowl, the far face stays plane
        out = xg.copy()
        yy, zz = xg[:, 1] / L - 0.5, xg[:, 2] / L - 0.5
        out[:, 0] = xg[:, 0] + 0.15 * (L / num_element) * 4 * (yy * yy + zz * zz) * (1.0 - xg[:, 0] / L)
        return out

    mesh = boxmesh.BoxMesh(P, num_element, grid=grid, rank=rank, length=L, dtype=float_type, warp=bowl)
    medium, fastest = None, speed_of_sound
    if a.nodal_lens:
        # callables of position: every rank evaluates them at its own dofs, ghosts included, so the values agree across ranks
        centre, r2 = 0.5 * np.asarray(mesh.length), (L / 6.0) ** 2
        bump = lambda xyz: np.exp(-np.sum((xyz - centre) ** 2, axis=1) / r2)  # noqa: E731
        medium = fusgpu_loader.submodule("nodal_medium").NodalMedium(
            lambda xyz: speed_of_sound + 300.0 * bump(xyz), lambda xyz: density + 200.0 * bump(xyz),
            nonlinear_coefficient=lambda xyz: nonlinear_coefficient + 1.5 * bump(xyz),
            attenuation_coefficient_dB=lambda xyz: attenuation_coefficient_dB + 4.8 * bump(xyz))
        fastest = speed_of_sound + 300.0  # the time-step rule takes the fastest speed of the medium
    h = ls.time_step_parameters(mesh, P, speed_of_sound, source_frequency, L)
    if world > 1:
        hm = torch.tensor([h], dtype=torch.float64, device="cuda")
        dist.all_reduce(hm, op=dist.ReduceOp.MIN)  # comm.Allreduce(hmin, mesh_size, op=MPI.MIN), :108
        h = float(hm.item())
    # :119-125 (CFL 0.40, an integer number of steps per period, final time L/c + 8/f)
    CFL = 0.40
    dt = CFL * h / (fastest * P**2)
    step_per_period = int(period / dt) + 1
    dt = period / step_per_period
    tf = L / speed_of_sound + 8.0 / source_frequency
    nstep = int(tf / dt) + 1
    if rank == 0:
        print(f"Number of steps: {nstep}", flush=True)
        print(f"Number of steps per period: {step_per_period}", flush=True)
        print(f"Number of degrees-of-freedom: {mesh.ndofs_global}", flush=True)
    source = None
    if a.array:
        src = fusgpu_loader.submodule("sources")
        ny, nz = (int(v) for v in a.array.split(","))
        focus = np.array([float(v) for v in a.focus.split(",")] if a.focus else [0.5 * L] * 3)
        # the elements split the face by the (y, z) of the facet centroids; their centres lie on the bowl
        centres = bowl(src.grid_centres(ny, nz, 0.0, (0.0, L), (0.0, L)))
        source = src.SourceArray(src.grid_elements(ny, nz, (0.0, L), (0.0, L)), delay=src.focus_delays(centres, focus, speed_of_sound),
                                 n_elements=ny * nz)
        if rank == 0:
            print(f"Array elements: {ny} x {nz}, focus: {tuple(float(v) for v in focus)}", flush=True)
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
        sponge = sp.SpongeLayer(sp.box_profile((0.0, 0.0, 0.0), mesh.length, a.sponge * L / num_element, sp.LATERAL, speed_of_sound))
    relaxation = None
    if a.power_law:
        rx = fusgpu_loader.submodule("relaxation")
        fit = rx.fit_power_law(a.power_law[0], a.power_law[1], 0.5 * source_frequency, 5.0 * source_frequency, n=2,
                               speed_of_sound=speed_of_sound, with_thermoviscous=True)
        relaxation = rx.RelaxationAbsorption(fit.tau, fit.kappa)
        try:
            relaxation.check_time_step(dt)  # a coarse mesh steps past the fastest mechanism
        except ValueError as e:
            raise SystemExit(f"--power-law: {e}") from None
        # the fitted diffusivity as the solver's attenuation coefficient at the source frequency (compute_diffusivity_of_sound, inverted)
        w0 = 2.0 * np.pi * source_frequency
        attenuation_coefficient_dB = fit.delta * w0 * w0 / (2.0 * speed_of_sound**3) * 20.0 / np.log(10.0)
        if rank == 0:
            print(f"Power law {a.power_law[0]:g} dB/cm/MHz^{a.power_law[1]:g}: tau = {fit.tau}, kappa = {fit.kappa}, delta = {fit.delta:.4g} "
                  f"(thermoviscous part {attenuation_coefficient_dB:.4g} dB/m at f0), largest relative error of the fit {fit.max_rel_error:.4f}",
                  flush=True)
    capture = None
    if a.shock_capture is not None:
        sc = fusgpu_loader.submodule("shock_capture")
        capture = sc.ShockCapture() if a.shock_capture < 0.0 else sc.ShockCapture(strength=a.shock_capture)
    solver = nls.WesterveltSpectral3D(mesh, float_type, speed_of_sound, density, source_frequency, source_amplitude,
                                      nonlinear_coefficient, attenuation_coefficient_dB, comm=comm, fused=not a.reference_sequence, source=source,
                                      sponge=sponge, relaxation=relaxation, nodal_medium=medium, shock_capture=capture,
                                      in_kernel_geometry=True if (a.in_kernel_geometry or a.geometry == "kernel") else ("auto" if a.geometry == "auto" else False))
    solver.init()
    if medium is not None and rank == 0:
        print(f"Nodal medium: c {solver.c_nodal.min():.1f} .. {solver.c_nodal.max():.1f} m/s, rho {solver.rho_nodal.min():.1f} .. "
              f"{solver.rho_nodal.max():.1f} kg/m^3, beta {solver.beta_nodal.min():.2f} .. {solver.beta_nodal.max():.2f}, alpha "
              f"{solver.att_nodal.min():.2f} .. {solver.att_nodal.max():.2f} dB/m at the dofs; cell pass: {solver.nodal_cell_pass if solver.fused else 'two launches (reference sequence)'}", flush=True)
    if sponge is not None:
        n_layer = solver._sponge[0].numel()
        print(f"Sponge layer (rank {rank}): {a.sponge} cell(s) wide, {n_layer} owned dofs, sigma_max dt = {sponge.sigma_max * dt:.3f}", flush=True)

    # sampling set: the owned dofs on the mid-z plane of the global dof grid
    lex = mesh.global_lexicographic_ids()[: mesh.nlocal]
    gd = mesh.global_dof_dims
    on_plane = np.nonzero((lex % gd[2]) == gd[2] // 2)[0]
    xyz = mesh.dof_coordinates()[: mesh.nlocal][on_plane]
    data = np.zeros((on_plane.size, 3))
    data[:, 0], data[:, 1] = xyz[:, 0], xyz[:, 1]
    if a.out_dir and rank == 0:
        os.makedirs(a.out_dir, exist_ok=True)
    if world > 1:
        dist.barrier()

    if a.stable_dt:
        dt_op = solver.stable_time_step(0.8)
        if rank == 0:
            print(f"Stable step from the operators: {dt_op:.6e} s at safety 0.8 (limit {solver.stable_limit:.6e} s: lambda_max "
                  f"{solver.lambda_max:.4e}, damping_max {solver.damping_max:.4e}); snapped CFL step: {dt:.6e} s", flush=True)
    energy = None
    if a.energy or a.guard:  # every rk4 call of the run paths below carries the two diagnostics (their cadence spans the calls)
        diag = fusgpu_loader.submodule("diagnostics")
        energy = diag.EnergyRecorder(solver, every=a.energy, capacity=nstep // a.energy + 1) if a.energy else None
        solver.rk4 = functools.partial(solver.rk4, energy=energy, guard=diag.FieldGuard(every=a.guard) if a.guard else None)

    def report_energy():
        if capture is not None:  # (every run path ends here)
            eps = capture.artificial_diffusivity()
            print(f"Shock capture (rank {rank}): {capture.active_cells()} of {mesh.ncells} cells active after {capture.launches} sensor "
                  f"launches, largest artificial diffusivity {eps.max() if eps.size else 0.0:.4e} m^2/s (at most "
                  f"{capture.eps_max.max():.4e}; physical {solver.delta:.4e})", flush=True)
        if energy is None:
            return
        te, kin, pot, tot, amax, bad = energy.energies()
        if rank == 0 and len(te):
            name = os.path.join(a.out_dir or ".", "energy.npz")
            np.savez(name, t=te, kinetic=kin, potential=pot, total=tot, absmax=amax, nonfinite=bad)
            print(f"Energy of the linear part: {len(te)} records, first {tot[0]:.6e} (t = {te[0]:.4e}), last {tot[-1]:.6e} "
                  f"(t = {te[-1]:.4e}) -> {name}", flush=True)

    a.report_energy = report_energy  # (the run paths below report before they take the process group down)
    if rank == 0:
        print("Solve!", flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t_collect = L / speed_of_sound + 6.0 / source_frequency  # :662
    budget = a.max_steps if a.max_steps is not None else nstep
    if a.sensor_plane:
        run_with_sensors(a, solver, mesh, comm, rank, world, L, float_type, t0, tf, dt, nstep, budget, t_collect, step_per_period,
                         source_frequency)
        return
    if a.field_stats or a.thermal or a.intensity:
        run_with_monitor(a, solver, mesh, comm, rank, world, float_type, t0, tf, dt, nstep, budget, t_collect, step_per_period,
                         source_frequency)
        return
    # up to the collection window in one go (no host round trip per step), then step by step with one dump per step
    n_before = min(budget, max(0, int(np.floor(t_collect / dt)) - 1))  # t stays <= the threshold: no dump is skipped
    t, steps = solver.rk4(0.0, tf, dt, max_steps=n_before) if n_before > 0 else (0.0, 0)
    step_period = 0
    while t < tf and steps < budget:
        t, more = solver.rk4(t, tf, dt, max_steps=1)
        steps += more
        if steps % 100 == 0 and rank == 0:
            print(f"t: {t:5.5},\t Steps: {steps}/{nstep}", flush=True)
        if t > t_collect and step_period < step_per_period:
            if a.out_dir:
                data[:, 2] = solver.u_sol()[on_plane]
                with open(os.path.join(a.out_dir, f"pressure_field_{step_period}.txt"), "a") as f:
                    np.savetxt(f, data, fmt="%.8f", delimiter=",")  # the reference's format, :675
            step_period += 1
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if rank == 0:
        print(f"t: {t:5.5},\t Steps: {steps}/{nstep}", flush=True)
        print(f"Fields collected over the last period: {step_period}/{step_per_period}")
        print(f"Solve time: {el}")
        print(f"Solve time per step: {el / max(steps, 1)}")
    report_energy()
    if world > 1:
        dist.destroy_process_group()


def run_with_sensors(a, solver, mesh, comm, rank, world, L, float_type, t0, tf, dt, nstep, budget, t_collect, step_per_period, f0):
    """The whole run in ONE rk4 call with point sensors recording the last period on the device (no full-field copy per step)."""
    import torch
    import torch.distributed as dist

    import fusgpu_loader

    sens = fusgpu_loader.submodule("sensors")
    nx, ny = (int(v) for v in a.sensor_plane.split(","))
    X, Y = np.meshgrid(np.linspace(0.0, L, nx), np.linspace(0.0, L, ny), indexing="ij")
    points = np.stack([X.reshape(-1), Y.reshape(-1), np.full(X.size, 0.5 * L)], axis=1)
    s = sens.PointSensors(mesh, points, float_type, capacity=step_per_period, peak=bool(a.peak_out),
                          harmonics=(1, 2) if a.peak_out else (), frequency=f0)
    t, steps = solver.rk4(0.0, tf, dt, max_steps=budget, sensors=s, record_from=t_collect)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    series = s.series()
    # every rank's points merged over the global list (a point on a face shared by two ranks: the lower rank's value)
    merged = s.gather(comm, series) if world > 1 else sens.merge([(s.point_ids, series)], points.shape[0])
    located = np.nonzero(~np.isnan(merged[0]))[0] if merged.shape[0] else np.zeros(0, np.int64)
    if rank == 0:
        print(f"t: {t:5.5},\t Steps: {steps}/{nstep}", flush=True)
        print(f"Fields collected over the last period: {s.nrec}/{step_per_period}")
        print(f"Sensor points on this plane: {located.size}/{points.shape[0]}")
        print(f"Solve time: {el}")
        print(f"Solve time per step: {el / max(steps, 1)}")
        data = np.zeros((located.size, 3))
        data[:, 0], data[:, 1] = points[located, 0], points[located, 1]
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            for k in range(merged.shape[0]):
                data[:, 2] = merged[k, located]
                with open(os.path.join(a.out_dir, f"pressure_field_{k}.txt"), "a") as f:
                    np.savetxt(f, data, fmt="%.8f", delimiter=",")  # the reference's format, :675
    if a.peak_out:
        pmax, pmin = s.peak()
        cols = np.stack([pmax, pmin, s.harmonic_amplitude(1), s.harmonic_amplitude(2)])  # [4, m]
        allc = s.gather(comm, cols) if world > 1 else sens.merge([(s.point_ids, cols)], points.shape[0])
        if rank == 0:
            keep = np.nonzero(~np.isnan(allc[0]))[0]
            rows = np.column_stack([points[keep, 0], points[keep, 1], allc[:, keep].T])
            np.savetxt(a.peak_out, rows, fmt="%.8f", delimiter=",")
    a.report_energy()
    if world > 1:
        dist.destroy_process_group()


def run_with_monitor(a, solver, mesh, comm, rank, world, float_type, t0, tf, dt, nstep, budget, t_collect, step_per_period, f0):
    """The whole run in ONE rk4 call with a full-field monitor accumulating the last period on the device: the maps the reference
    post-processes from its per-step dumps (cuda/demo_nonlinear_bowl.py:662-680), without a field copy per step."""
    import torch
    import torch.distributed as dist

    import fusgpu_loader

    fm = fusgpu_loader.submodule("field_monitor")
    m = fm.FieldMonitor(mesh.nlocal, float_type, peak=True, mean_square=("u", "v"), harmonics=(1, 2), frequency=f0)
    # one period and no more: the run stops steps_per_period steps after the first one that ends after t_collect
    ends = [e for e in fm.record_times(0.0, tf, dt, budget) if not e > t_collect]
    t, steps = solver.rk4(0.0, tf, dt, max_steps=min(budget, len(ends) + step_per_period), monitor=m, record_from=t_collect)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = {"nacc": m.nacc, "steps_per_period": step_per_period, "lexicographic_ids": mesh.global_lexicographic_ids()[: mesh.nlocal]}
    if m.nacc:
        h1 = m.harmonic_amplitude(1)
        foc = fm.focus(h1, solver, 0.5, comm if world > 1 else None)
        host = lambda x: x.cpu().numpy()  # noqa: E731
        out.update(pmax=host(m.peak()[0]), pmin=host(m.peak()[1]), H1=host(h1), H2=host(m.harmonic_amplitude(2)),
                   u_mean_square=host(m.mean_square("u")), q=host(_heat_deposition(m, solver)), focus_max=foc["max"], focus_dof=foc["dof"],
                   focus_rank=foc["rank"], focus_position=np.asarray(foc["position"] if foc["position"] is not None else [np.nan] * 3),
                   focus_volume=foc["volume"], focus_level=foc["level"])
    if a.field_stats:
        name = a.field_stats if world == 1 else f"{os.path.splitext(a.field_stats)[0]}.rank{rank}.npz"
        np.savez(name, **out)
    if rank == 0:
        print(f"t: {t:5.5},\t Steps: {steps}/{nstep}", flush=True)
        print(f"Fields accumulated over the last period: {m.nacc}/{step_per_period}")
        if m.nacc:
            print(f"Focus of |H1|: {out['focus_max']:.6g} Pa at {tuple(out['focus_position'])}, -6 dB volume {out['focus_volume']:.6g} m^3")
        print(f"Solve time: {el}")
        print(f"Solve time per step: {el / max(steps, 1)}")
    if a.intensity and m.nacc:
        run_intensity(solver, m, comm, rank, world)
    if a.thermal and m.nacc:
        run_thermal(a, solver, m, mesh, comm, rank, world, float_type)
    a.report_energy()
    if world > 1:
        dist.destroy_process_group()


def _heat_deposition(monitor, solver):
    """The absorbed power density of the last period: with --power-law the mechanisms' part beside the thermoviscous one."""
    if solver.relaxation is None:
        return monitor.heat_deposition(solver)
    import fusgpu_loader

    return fusgpu_loader.submodule("relaxation").heat_deposition(monitor, solver)


def run_intensity(solver, monitor, comm, rank, world):
    """The intensity vector and the radiation force density of the last period, from the monitor's harmonic maps and the gradient
    operator (intensity.py); nothing leaves the device but the printed figures."""
    import fusgpu_loader

    fm, it = fusgpu_loader.submodule("field_monitor"), fusgpu_loader.submodule("intensity")
    reduce = comm if world > 1 else None
    mag_i = it.magnitude(monitor.intensity(solver))
    foc = fm.focus(mag_i, solver, 0.5, reduce)
    # beside it, for the reader: what a plane wave of the focal first-harmonic amplitude would carry (no check: a focus is not one)
    p1 = fm.focus(monitor.harmonic_amplitude(1), solver, 0.5, reduce)["max"]
    plane = p1 * p1 / (2.0 * float(np.mean(solver.rho_cells)) * float(np.mean(solver.c_cells)))
    force = fm.focus(it.magnitude(monitor.radiation_force(solver)), solver, 0.5, reduce)
    if rank == 0:
        print(f"Focus of |I|: {foc['max']:.6g} W/m^2 at {foc['position']}, -6 dB volume {foc['volume']:.6g} m^3")
        print(f"Plane-wave estimate p1^2 / (2 rho c) at the focus of |H1|: {plane:.6g} W/m^2")
        print(f"Peak |F|: {force['max']:.6g} N/m^3 at {force['position']}")


def run_thermal(a, solver, monitor, mesh, comm, rank, world, float_type):
    """Pressure -> heat -> temperature -> dose on the same mesh and partition: the heat deposition of the last period drives Pennes'
    equation (soft tissue, insulated boundaries) for SECONDS_ON, then the tissue cools for SECONDS_OFF; nothing leaves the device
    but the printed figures."""
    import fusgpu_loader

    fm, bh = fusgpu_loader.submodule("field_monitor"), fusgpu_loader.submodule("bioheat")
    th = bh.BioheatSpectral3D(mesh, float_type, comm=comm)
    th.set_heat_source(bh.heat_source_from(monitor, solver, th) if solver.relaxation is None else _heat_deposition(monitor, solver).to(th.tdt))
    dt = th.stable_time_step()
    t_on, t_off = a.thermal[0], (a.thermal[1] if len(a.thermal) > 1 else 0.0)
    t, steps = th.advance(0.0, t_on, dt)
    if t_off > 0.0:
        t, more = th.advance(t_on, t_on + t_off, dt, power=(0.0, 0.0))
        steps += more
    reduce = comm if world > 1 else None
    peak = fm.focus(th.peak_temperature(), th, 1.0, reduce)
    dose = fm.focus(th.cem43(), th, 0.5, reduce)
    lesion = fm.focus(th.cem43(), th, 240.0 / dose["max"], reduce)["volume"] if dose["max"] >= 240.0 else 0.0
    if rank == 0:
        print(f"Thermal steps: {steps} of {dt:.6g} s ({t_on:g} s on, {t_off:g} s off)")
        print(f"Focus of cem43: {dose['max']:.6g} min at {dose['position']}, half-maximum volume {dose['volume']:.6g} m^3")
        print(f"thermal: peak temperature={peak['max']:.6f} degC, max cem43={dose['max']:.6g} min, volume above 240 cem43={lesion:.6g} m^3")


if __name__ == "__main__":
    main()
