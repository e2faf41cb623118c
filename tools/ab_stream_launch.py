#!/usr/bin/env python3
"""Two builds of libfusgpu.so (the parent commit's and this tree's) loaded into ONE process, arms alternating: every streaming launcher
(csrc/stream_shape.hpp) through the C ABI at config-3 size (10 218 313 dofs) and at a launch-bound size (4 099 dofs), and the mass gather
on the dofmaps of a 54^3 and a 6^3 mesh (one workspace, built by both libraries in turn: both arms read the same addresses).  Before
timing, each case runs once per library on the same inputs and the outputs are compared bit for bit.  Exit status 1 if any differ.

    python tools/ab_stream_launch.py PARENT_LIB HEAD_LIB [--log profiles/NAME.log] [--only-mass]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))



def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_lib")
    ap.add_argument("head_lib")
    ap.add_argument("--log", default="")
    ap.add_argument("--only-mass", action="store_true")
    a = ap.parse_args(argv)
    import numpy as np
    import torch

    import fusgpu_loader
    import measure

    lib_mod = fusgpu_loader.submodule("_lib")

    torch.cuda.set_device(0)
    libs = {arm: lib_mod.bind(C.CDLL(os.path.abspath(path))) for arm, path in (("parent", a.parent_lib), ("head", a.head_lib))}
    sp = lib_mod.stream_ptr
    with measure.Log("ab_stream_launch", a.log) as log:
        log(f"# tools/ab_stream_launch.py on {torch.cuda.get_device_name(0)}: parent library {libs['parent'].fus_source_hash().decode()}, "
            f"head library {libs['head'].fus_source_hash().decode()}; arms alternate in one process, median of 7 rounds, bar = 3 x the larger spread")
        bad = 0

        def case(name, bufs, call, reps, rounds=7, host=False):
            """call(lib) launches once.  bufs: every tensor the launch may write."""
            nonlocal bad
            saved = [t.clone() for t in bufs]
            outs = {}
            for arm, lib in libs.items():
                for t, s in zip(bufs, saved):
                    t.copy_(s)
                rc = call(lib)
                torch.cuda.synchronize()
                assert rc == 0, (name, arm, rc)
                outs[arm] = [t.clone() for t in bufs]
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs["parent"], outs["head"]))
            bad += not same
            for t, s in zip(bufs, saved):
                t.copy_(s)
            del outs, saved
            arms = {arm: (lambda lib=lib: call(lib)) for arm, lib in libs.items()}
            res = measure.interleave(arms, rounds, lambda fn: measure.event_time(fn, reps), warm=100, alternate=True)
            med = {k: measure.stats(v) for k, v in res.items()}
            log(f"{name:58s} bitwise {'equal' if same else 'DIFFERENT'}  parent {med['parent'].median * 1e3:8.2f} us  head {med['head'].median * 1e3:8.2f} us")
            for line in measure.verdict_lines(res, to_us=1e3):
                log(line)
            if host:
                hres = measure.interleave(arms, rounds, lambda fn: measure.host_time(lambda: [fn() for _ in range(reps)], reps), alternate=True)
                hm = {k: measure.stats(v) for k, v in hres.items()}
                log(f"{name + ', host clock per launch':58s}                parent {hm['parent'].median * 1e3:8.2f} us  head {hm['head'].median * 1e3:8.2f} us")
                for line in measure.verdict_lines(hres, to_us=1e3):
                    log(line)

        for n, reps, host in () if a.only_mass else ((10218313, 200, False), (4099, 2000, True)):
            for tdt, suf in ((torch.float64, "f64"), (torch.float32, "f32")):
                if n < 100000 and suf == "f32":
                    continue
                tag = f"n={n} {suf}"
                vec = [(torch.rand(n + 4, dtype=torch.float64, device="cuda") + 1).to(tdt) for _ in range(11)]
                al = [v[:n] for v in vec]      # 16-byte aligned
                sh = [v[1:n + 1] for v in vec]  # shifted by one element
                p, q = [v.data_ptr() for v in al], [v.data_ptr() for v in sh]
                f = lambda lib, nm: getattr(lib, f"fus_{nm}_{suf}")  # noqa: E731
                case(f"{tag} axpy", [al[1]], lambda L: f(L, "axpy")(0.5, p[0], p[1], n, sp()), reps, host=host)
                case(f"{tag} axpy, shifted operands", [sh[1]], lambda L: f(L, "axpy")(0.5, q[0], q[1], n, sp()), reps)
                case(f"{tag} copy", [al[1]], lambda L: f(L, "copy")(p[0], p[1], n, sp()), reps)
                case(f"{tag} fill", [al[1]], lambda L: f(L, "fill")(1.0, p[1], n, sp()), reps, host=host)
                case(f"{tag} muladd", [al[2]], lambda L: f(L, "muladd")(p[0], p[1], p[2], n, sp()), reps)
                for kind in range(8):
                    case(f"{tag} rk4_stage kind {kind}", al[1:8], lambda L: f(L, "rk4_stage")(1e-9, 1e-9, kind, *p[:8], n - 7, n, sp()), reps, host=host and kind == 0)
                case(f"{tag} rk4_stage kind 0, shifted operands", sh[1:8], lambda L: f(L, "rk4_stage")(1e-9, 1e-9, 0, *q[:8], n - 7, n, sp()), reps)
                for kind in range(8):
                    case(f"{tag} rk4_stage_nl2 kind {kind}", al[3:11], lambda L: f(L, "rk4_stage_nl2")(1e-9, 1e-9, kind, *p[:10], 0.25, p[10], n - 7, n, sp()), reps,
                         host=host and kind == 0)
                    case(f"{tag} rk4_stage_nl2 kind {kind}, no w", al[3:11], lambda L: f(L, "rk4_stage_nl2")(1e-9, 1e-9, kind, *p[:10], 0.25, None, n - 7, n, sp()), reps)
                case(f"{tag} rk4_stage_nl2 kind 0, shifted operands", sh[3:11], lambda L: f(L, "rk4_stage_nl2")(1e-9, 1e-9, 0, *q[:10], 0.25, q[10], n - 7, n, sp()), reps)
                for kind in range(4):
                    case(f"{tag} rk4_stage_nl kind {kind}", al[1:9], lambda L: f(L, "rk4_stage_nl")(1e-9, 1e-9, kind, *p[:9], n - 7, n, sp()), reps, host=host and kind == 0)
                # bioheat: minv pr s b T0 Tn acc | cem43 tmax
                cem = torch.zeros(n, dtype=torch.float64, device="cuda")
                for kind, nm in ((0, "FIRST"), (2, "LAST")):
                    case(f"{tag} bioheat {nm}", al[3:8] + [cem],
                         lambda L: f(L, "bioheat_stage")(1e-9, 1e-9, kind, 1.0, 37.0, 1e-9, *p[:7], cem.data_ptr(), p[7], 0, n - 7, n, sp()), reps,
                         host=host and kind == 2)
                case(f"{tag} bioheat LAST, shifted operands", sh[3:8] + [cem],
                     lambda L: f(L, "bioheat_stage")(1e-9, 1e-9, 2, 1.0, 37.0, 1e-9, *q[:7], cem.data_ptr(), q[7], 0, n - 7, n, sp()), reps)
                # field monitor: u v | pmax pmin usq vsq hre him
                usq, vsq = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
                hstride = (n + 1) // 2 * 2
                hre, him = (torch.zeros(4 * hstride, dtype=torch.float64, device="cuda") for _ in range(2))
                coef = torch.rand(8, dtype=torch.float64, device="cuda")
                for H in (0, 4):
                    case(f"{tag} field_accumulate peak + usq + vsq, H = {H}", [al[2], al[3], usq, vsq, hre, him],
                         lambda L: f(L, "field_accumulate")(p[0], p[1], n, p[2], p[3], usq.data_ptr(), vsq.data_ptr(), hre.data_ptr() if H else None,
                                                            him.data_ptr() if H else None, hstride, coef.data_ptr(), H, 0, sp()), reps, host=host and H == 4)
                del vec, al, sh, cem, usq, vsq, hre, him
                torch.cuda.empty_cache()

        # mass gather and its static-detJ form on the dofmap of config 3 (P = 4, 54^3 cells) and of a 6^3 mesh; one plan built by both libraries
        boxmesh = fusgpu_loader.submodule("boxmesh")
        for cells, reps in ((54, 200), (6, 2000)):
            mesh = boxmesh.BoxMesh(4, cells)
            dm = torch.from_numpy(np.ascontiguousarray(mesh.dofmap)).cuda()
            nent, N = dm.shape
            nd = mesh.ndofs
            for tdt, suf in ((torch.float64, "f64"), (torch.float32, "f32")):
                x = torch.rand(nd, dtype=torch.float64, device="cuda").to(tdt)
                cc = (torch.rand(nent, dtype=torch.float64, device="cuda") + 0.5).to(tdt)
                detJ = (torch.rand(nent, N, dtype=torch.float64, device="cuda") + 0.5).to(tdt)
                y = torch.zeros(nd, dtype=tdt, device="cuda")
                # ONE workspace and ONE static companion, built by each library in turn (each registers the pointer; the contents are the
                # same): the arms then read the same addresses
                ws = sws = None
                for arm, L in libs.items():
                    nb = L.fus_mass_gather_plan_bytes(N, nent, nd)
                    ws = torch.empty(int(nb), dtype=torch.uint8, device="cuda") if ws is None else ws
                    assert L.fus_mass_gather_plan_build(dm.data_ptr(), N, nent, nd, ws.data_ptr(), int(nb), sp()) == 0
                    sb = L.fus_mass_gather_static_bytes(N, nent, x.element_size())
                    sws = torch.empty(int(sb), dtype=torch.uint8, device="cuda") if sws is None else sws
                    assert getattr(L, f"fus_mass_gather_static_build_{suf}")(ws.data_ptr(), detJ.data_ptr(), sws.data_ptr(), int(sb), sp()) == 0
                torch.cuda.synchronize()
                tag = f"P=4 {cells}^3 cells ({nd} dofs) {suf}"
                case(f"{tag} mass gather", [y],
                     lambda L: getattr(L, f"fus_mass_apply_gather_{suf}")(x.data_ptr(), cc.data_ptr(), y.data_ptr(), detJ.data_ptr(),
                                                                          ws.data_ptr(), N, nent, sp()), reps, host=cells == 6 and suf == "f64")
                case(f"{tag} mass gather, static detJ", [y],
                     lambda L: getattr(L, f"fus_mass_apply_gather_static_{suf}")(x.data_ptr(), cc.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                                                                 sws.data_ptr(), N, nent, sp()), reps)
        log(f"# cases whose outputs differ between the libraries: {bad}")
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
