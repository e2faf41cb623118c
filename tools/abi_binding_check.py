#!/usr/bin/env python3
"""The ctypes binding ``_lib.py`` derives from include/fus_gpu.h against an earlier, hand-written ``_lib.py`` (a file of that
revision, e.g. ``git show REV:fenicsx-fus-gpu_amd/_lib.py > /tmp/old_lib.py``): both bind the built library (no GPU needed) and
the ``argtypes`` / ``restype`` that end up on every function are compared, then the constants.  Exit status 1 on any difference.

    python tools/abi_binding_check.py OLD_LIB_PY [--log profiles/NAME.log]
"""
import argparse
import ctypes as C
import importlib.util
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

CONSTANTS = ("ABI_VERSION", "ERR_COMM", "ERR_UNSUPPORTED_ENTITY", "TUNE_STIFFNESS_VARIANT", "TUNE_XCD_REMAP", "TUNE_MASS_VARIANT",
             "TUNE_PLAN_VARIANT", "TUNE_PLAN_RUNS", "TUNE_VECTOR_STREAM", "TUNE_PLAN_ROWS", "TUNE_PLAN_XCD_GROUP", "UNIQUE_ID_BYTES",
             "FORK_LAZY", "FORK_ATTACH", "MIN_DEGREE", "MAX_DEGREE")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_lib_py")
    ap.add_argument("--log", default="")
    a = ap.parse_args(argv)
    import fusgpu_loader

    new = fusgpu_loader.submodule("_lib")
    os.environ["FUS_LIB_PATH"] = new.LIB_PATH  # the earlier module computes its default from its own location
    spec = importlib.util.spec_from_file_location("old_lib", a.old_lib_py)
    old = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(old)
    old_cdll, new_cdll = old.load(), new.bind(C.CDLL(new.LIB_PATH))  # two CDLL objects: each keeps its own function objects

    lines, diffs, retyped = [], 0, []

    def log(s):
        lines.append(s)
        print(s)

    def differs(s):
        nonlocal diffs
        diffs += 1
        log("DIFFERENCE: " + s)

    log(f"# tools/abi_binding_check.py: {os.path.basename(a.old_lib_py)} (hand-written table) against the binding parsed from include/fus_gpu.h")
    if list(old.SIGNATURES) != [n for n in old.SIGNATURES if n in new.SIGNATURES] or len(old.SIGNATURES) != len(new.SIGNATURES):
        differs(f"SIGNATURES names: {sorted(set(old.SIGNATURES) ^ set(new.SIGNATURES))}")
    log(f"SIGNATURES: {len(old.SIGNATURES)} names before, {len(new.SIGNATURES)} now")
    by_value = pointers = 0
    for name in sorted(set(old.SIGNATURES) & set(new.SIGNATURES)):
        o, n = old.SIGNATURES[name], new.SIGNATURES[name]
        if len(o) != len(n):
            differs(f"{name}: {len(o)} arguments before, {len(n)} now")
            continue
        if list(getattr(new_cdll, name).argtypes) != n or list(getattr(old_cdll, name).argtypes) != o:
            differs(f"{name}: argtypes on the bound function are not the SIGNATURES entry")
        for i, (to, tn) in enumerate(zip(o, n)):
            if to in (C.c_int, C.c_int64, C.c_double, C.c_float):
                by_value += 1
                if tn is not to:
                    differs(f"{name} argument {i}: {to.__name__} before, {tn.__name__} now")
            else:
                pointers += 1
                if tn is not C.c_void_p:
                    differs(f"{name} argument {i}: pointer {to.__name__} before, {tn.__name__} now")
                if to is not C.c_void_p:
                    retyped.append(f"{name} argument {i}: {to.__name__} -> c_void_p")
    log(f"arguments: {by_value} by value (identical class), {pointers} pointers (all c_void_p now)")
    log(f"typed pointers before, c_void_p now: {len(retyped)}")
    for r in retyped:
        log("  " + r)
    if len(retyped) != 12:
        differs(f"{len(retyped)} retyped pointer parameters, 12 expected")
    names = sorted(new.DECLARATIONS)
    other = []
    for name in names:
        ro, rn = getattr(old_cdll, name).restype, getattr(new_cdll, name).restype
        if ro is not rn:
            differs(f"{name}: restype {ro.__name__} before, {rn.__name__} now")
        if name not in new.SIGNATURES and list(getattr(old_cdll, name).argtypes) != list(getattr(new_cdll, name).argtypes):
            differs(f"{name}: argtypes (bound by hand before)")
        if rn is not C.c_int:
            other.append(f"{name} {rn.__name__}")
    log(f"return types: {len(names)} functions compared; not int: {', '.join(other)}")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fus_gpu.h")).read(), flags=re.S)
    for c in CONSTANTS:
        m = re.search(rf"^#define FUS_{c}\s+\(?(-?\d+)\)?\s*$", hdr, re.M)
        v = getattr(new, c)
        had = getattr(old, c, None)
        if m is None or int(m[1]) != v or (had is not None and had != v):
            differs(f"{c}: header {m and m[1]}, before {had}, now {v}")
        log(f"{c} = {v}  (header {m and m[1]}, before {'-' if had is None else had})")
    log(f"# {diffs} differences")
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
