#!/usr/bin/env python3
"""Kernel by kernel, is the device code of this tree the code of another tree (the parent commit, checked out beside it)?

    python tools/compare_kernels.py PARENT_TREE [regex ...]

Every translation unit of libfusgpu.so (resource_usage.UNITS) is compiled device-only to assembly in both trees with the Makefile's flags;
the output is split by kernel symbol and stripped of comment and directive lines (the rule of tests/test_kernel_isa.py).  A kernel whose
instruction list is equal is reported ``identical`` (branch targets without the number of the function in its unit, ``.LBB<function>_<block>``:
it changes when code is only moved between units); any other with the resource lines of both trees (kernel-resource-usage remarks,
resource_usage.parse) and the opcodes whose counts differ.  No GPU needed.  Exit status 1 if a kernel differs or exists in one tree only."""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resource_usage as ru  # noqa: E402

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=fast", "-fno-slp-vectorize",
         "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]


def compile_tree(root):
    """(assembly, remarks) of every unit of the tree at ``root``, cached under its csrc/_asm/compare keyed on source mtimes."""
    csrc = os.path.join(root, "fenicsx-fus-gpu_amd", "csrc")
    out = os.path.join(csrc, "_asm", "compare")
    os.makedirs(out, exist_ok=True)
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".hpp"))] + [p for p in (os.path.join(root, "include", h) for h in ("fus_gpu.h", "fus_gpu_array.h", "fus_gpu_relaxation.h", "fus_gpu_nodal.h", "fus_gpu_westervelt_nodal.h", "fus_gpu_waveform.h", "fus_gpu_reduce.h", "fus_gpu_sensor.h")) if os.path.exists(p)]
    newest = max(os.path.getmtime(p) for p in srcs)
    procs, files = [], []
    for src, defs in ru.UNITS:
        if not os.path.exists(os.path.join(csrc, src)):  # a unit the other tree does not have yet: its kernels are "only in" one tree
            continue
        stem = os.path.join(out, src[:-4] + "".join(d.replace("-DFUS_INST_T=", "_") for d in defs))
        files.append(stem)
        if os.path.exists(stem + ".s") and os.path.exists(stem + ".txt") and os.path.getmtime(stem + ".txt") >= newest:
            continue
        cmd = [ru.HIPCC, *FLAGS, *defs, "-o", stem + ".s", src]
        procs.append((cmd, stem, subprocess.Popen(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for cmd, stem, p in procs:
        _, err = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{err[-4000:]}")
        with open(stem + ".txt", "w") as f:
            f.write(err)
    return "".join(open(s + ".s").read() for s in files), "".join(open(s + ".txt").read() for s in files)


def split_kernels(asm):
    """{mangled name: [instruction lines]} of the symbols that are code (their text ends with s_endpgm; a data symbol of the namespace is none)"""
    found, cur = {}, None
    for ln in asm.split("\n"):
        m = re.match(r"^(_ZN3fus\w+):", ln)
        if m:
            cur = m.group(1)
            found[cur] = []
            continue
        if cur is not None:
            s = ln.strip()
            if s and not s.startswith((";", ".")):
                found[cur].append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s))
            if s.startswith("s_endpgm"):
                cur = None
    return {k: v for k, v in found.items() if v and v[-1].startswith("s_endpgm")}


def resources(d):
    return (f"VGPR {d['vgpr']:4d} AGPR {d['agpr']:3d} SGPR {d['sgpr']:4d} scratch {d['scratch']:4d} occ {d['occupancy']} LDS {d['lds']}"
            if d else "(no remark)")


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    pats = [re.compile(p) for p in sys.argv[2:]]
    asm_a, rem_a = compile_tree(os.path.abspath(sys.argv[1]))
    asm_b, rem_b = compile_tree(ru.ROOT)
    ka, kb = split_kernels(asm_a), split_kernels(asm_b)
    ra, rb = ru.parse(rem_a), ru.parse(rem_b)
    names = sorted(set(ka) | set(kb))
    same = diff = 0
    for mangled, name in zip(names, ru.demangle(names)):
        if pats and not any(p.search(name) for p in pats):
            continue
        short = re.sub(r"\(.*", "", name).replace("void fus::", "")
        if mangled not in ka or mangled not in kb:
            print(f"{short}: only in the {'parent' if mangled in ka else 'branch'}")
            diff += 1
        elif ka[mangled] == kb[mangled]:
            print(f"{short}: identical ({len(ka[mangled])} instructions)")
            same += 1
        else:
            diff += 1
            ca, cb = (collections.Counter(s.split()[0] for s in k[mangled]) for k in (ka, kb))
            ops = ", ".join(f"{op} {cb[op] - ca[op]:+d}" for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op])
            print(f"{short}: DIFFERS\n    parent {resources(ra.get(name))}  {len(ka[mangled])} instructions\n"
                  f"    branch {resources(rb.get(name))}  {len(kb[mangled])} instructions\n"
                  f"    opcode counts: {ops or 'equal (same multiset, another order or other registers)'}")
    print(f"# {same} kernels identical, {diff} not")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
