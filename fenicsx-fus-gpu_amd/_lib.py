"""
ctypes binding of ``csrc/libfusgpu.so`` (C ABI declared in include/fus_gpu.h).

There is no CPU fallback: if the HIP library has not been built, or no GPU is
visible when a kernel is requested, this module raises.
"""

from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# FUS_LIB_PATH: load another build of the same ABI (A/B runs of two builds on one device)
LIB_PATH = os.environ.get("FUS_LIB_PATH") or os.path.join(_HERE, "csrc", "libfusgpu.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fus_gpu.h")
# headers that extend the ABI with further entry points of the same library (each includes fus_gpu.h): additions since the set of
# functions of fus_gpu.h was pinned are declared there, and bound from there in the same way
EXTENSION_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "fus_gpu_array.h"),)
# ... and the headers added since THAT set was pinned in its turn (tests/test_point_sources.py pins EXTENSIONS to fus_gpu_array.h's four
# functions): every later extension header goes here, its functions into ADDITIONS
ADDITION_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "fus_gpu_relaxation.h"),)
# ... and, ADDITIONS being pinned too (tests/test_relaxation.py), the open tier: the path of EVERY later header is appended here, its
# functions land in LATER, and no test pins that set to what it holds today
LATER_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "fus_gpu_nodal.h"),
                      os.path.join(os.path.dirname(_HERE), "include", "fus_gpu_westervelt_nodal.h"),
                      os.path.join(os.path.dirname(_HERE), "include", "fus_gpu_reduce.h"),
                      os.path.join(os.path.dirname(_HERE), "include", "fus_gpu_sensor.h"),
                      os.path.join(os.path.dirname(_HERE), "include", "fus_gpu_waveform.h"))  # (tests/test_waveform_sources.py: the last)


class FusGpuError(RuntimeError):
    pass


_BY_VALUE = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const char*": C.c_char_p}


def parse_header(text):
    """The C ABI as include/fus_gpu.h declares it -> ({function: (restype, [argtypes])}, {macro: integer value}).
    Every pointer, and a handle (``typedef struct X* name;``) by value, is ``c_void_p``; a scalar by value is its ctypes class.
    Anything else is refused, never guessed: a wrong class here would hand a kernel launch garbage instead of failing to load."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m[0].count("\n"), text, flags=re.S)  # comments, keeping the line structure
    defines = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(FUS_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)  # the other preprocessor lines: include guard, #include, #ifdef __cplusplus
    text = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', "", text, flags=re.M)
    functions, handles = {}, set()
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        handle = re.fullmatch(r"typedef struct \w+ ?\* ?(\w+)", stmt)
        if handle:
            handles.add(handle[1])
            continue
        if not stmt:
            continue
        m = re.fullmatch(r"([\w\s*]+?) ?\b(fus_\w+) ?\(([^()]*)\)", stmt)
        ret = m and m[1].replace(" *", "*")
        if not m or ret not in _RETURNS:
            raise FusGpuError(f"include/fus_gpu.h: cannot bind '{stmt[:120]}': not a prototype 'int | int64_t | void* | const char* fus_name(parameters)'")
        params = [] if m[3].strip() in ("", "void") else m[3].split(",")
        argtypes = []
        for p in params:
            words = [w for w in p.split() if w != "const"]  # type, then the name if there is one
            if "*" in p or (1 <= len(words) <= 2 and words[0] in handles and words[-1].isidentifier()):
                argtypes.append(C.c_void_p)
            elif 1 <= len(words) <= 2 and words[0] in _BY_VALUE and words[-1].isidentifier():
                argtypes.append(_BY_VALUE[words[0]])
            else:
                raise FusGpuError(f"include/fus_gpu.h: {m[2]}: parameter '{p.strip()}' is neither a pointer, a handle nor one of {', '.join(_BY_VALUE)} by value")
        functions[m[2]] = (_RETURNS[ret], argtypes)
    return functions, defines


def _read_header(path=None):
    path = HEADER_PATH if path is None else path
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise FusGpuError(f"{path}: the C ABI's header, which this binding is derived from, cannot be read ({e})") from None


# every function include/fus_gpu.h declares, and its integer macros: the header is the one declaration, nothing is restated here
DECLARATIONS, _DEFINES = _read_header()
# {name: argtypes} of the entry points (what a stand-in library has to answer); the two that only return a string are bound like the rest
SIGNATURES = {name: argtypes for name, (_, argtypes) in DECLARATIONS.items() if name not in ("fus_error_string", "fus_source_hash")}

# ... and every function the extension headers declare, {name: (restype, [argtypes])}: bound with the rest, kept apart from them
EXTENSIONS = {name: decl for path in EXTENSION_HEADER_PATHS for name, decl in _read_header(path)[0].items()}
if set(EXTENSIONS) & set(DECLARATIONS):
    raise FusGpuError(f"declared both in include/fus_gpu.h and in an extension header: {sorted(set(EXTENSIONS) & set(DECLARATIONS))}")
ADDITIONS = {name: decl for path in ADDITION_HEADER_PATHS for name, decl in _read_header(path)[0].items()}
if set(ADDITIONS) & (set(EXTENSIONS) | set(DECLARATIONS)):
    raise FusGpuError(f"declared in two headers of the C ABI: {sorted(set(ADDITIONS) & (set(EXTENSIONS) | set(DECLARATIONS)))}")


def declared_later(paths, earlier):
    """{name: (restype, [argtypes])} of the functions the headers at ``paths`` declare; a name that ``earlier`` (the names of the
    tiers before) or a header before it in ``paths`` holds already is refused."""
    tier = {}
    for path in paths:
        functions = _read_header(path)[0]
        twice = set(functions) & (set(earlier) | set(tier))
        if twice:
            raise FusGpuError(f"declared in two headers of the C ABI: {sorted(twice)} ({path})")
        tier.update(functions)
    return tier


LATER = declared_later(LATER_HEADER_PATHS, set(DECLARATIONS) | set(EXTENSIONS) | set(ADDITIONS))

ABI_VERSION = _DEFINES["FUS_ABI_VERSION"]
ERR_COMM = _DEFINES["FUS_ERR_COMM"]
ERR_UNSUPPORTED_ENTITY = _DEFINES["FUS_ERR_UNSUPPORTED_ENTITY"]
MIN_DEGREE, MAX_DEGREE = _DEFINES["FUS_MIN_DEGREE"], _DEFINES["FUS_MAX_DEGREE"]
UNIQUE_ID_BYTES = _DEFINES["FUS_UNIQUE_ID_BYTES"]
FORK_LAZY, FORK_ATTACH = _DEFINES["FUS_FORK_LAZY"], _DEFINES["FUS_FORK_ATTACH"]
# tuning keys: the header documents each next to its #define
TUNE_STIFFNESS_VARIANT = _DEFINES["FUS_TUNE_STIFFNESS_VARIANT"]
TUNE_XCD_REMAP = _DEFINES["FUS_TUNE_XCD_REMAP"]
TUNE_MASS_VARIANT = _DEFINES["FUS_TUNE_MASS_VARIANT"]
TUNE_PLAN_VARIANT = _DEFINES["FUS_TUNE_PLAN_VARIANT"]
TUNE_PLAN_RUNS = _DEFINES["FUS_TUNE_PLAN_RUNS"]
TUNE_VECTOR_STREAM = _DEFINES["FUS_TUNE_VECTOR_STREAM"]
TUNE_PLAN_ROWS = _DEFINES["FUS_TUNE_PLAN_ROWS"]
TUNE_PLAN_XCD_GROUP = _DEFINES["FUS_TUNE_PLAN_XCD_GROUP"]
TUNE_PLAN_SWEEP = _DEFINES["FUS_TUNE_PLAN_SWEEP"]

_lib = None


def bind(cdll):
    """Set ``argtypes`` and ``restype`` of every declared function (include/fus_gpu.h and its extension headers) on a loaded library;
    AttributeError if it lacks one."""
    for name, (restype, argtypes) in {**DECLARATIONS, **EXTENSIONS, **ADDITIONS, **LATER}.items():
        fn = getattr(cdll, name)
        fn.argtypes, fn.restype = argtypes, restype
    return cdll


def load():
    """Load libfusgpu.so (once). Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FusGpuError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C fenicsx-fus-gpu_amd/csrc`). "
            "There is no CPU fallback."
        )
    lib = bind(C.CDLL(LIB_PATH))
    if lib.fus_abi_version() != ABI_VERSION:
        raise FusGpuError(f"{LIB_PATH}: ABI version {lib.fus_abi_version()}, this package needs {ABI_VERSION} "
                          "(include/fus_gpu.h FUS_ABI_VERSION): rebuild the library")
    _lib = lib
    return lib


def tree_source_hash():
    """The hash csrc/Makefile embeds (fus_source_hash()), recomputed from the sources in this tree."""
    import hashlib

    csrc = os.path.join(_HERE, "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    names = re.search(r"^SRC = (.*)$", mk, re.M).group(1).split() + re.search(r"^HDR = (.*)$", mk, re.M).group(1).split()
    h = hashlib.sha256()
    for n in sorted(names):
        with open(os.path.join(csrc, n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def built_from_tree():
    """True if the loaded library was built from exactly the sources in this tree."""
    return load().fus_source_hash().decode() == tree_source_hash()


def check(rc: int, what: str = "", comm=None):
    if rc != 0:
        msg = load().fus_error_string(rc).decode()
        if rc == ERR_COMM:
            detail = load().fus_comm_last_error(comm)
            msg += ": " + (detail.decode() if detail else "?")
        elif comm is not None and rc == -1:  # a misuse the communicator explains (fork / join stream contract)
            detail = load().fus_comm_last_error(comm)
            if detail:
                msg += ": " + detail.decode()
        raise FusGpuError(f"{what or 'libfusgpu call'} failed: {msg} (code {rc})")


def torch_dtype(float_type):
    dt = np.dtype(float_type)
    if dt == np.float64:
        return torch.float64
    if dt == np.float32:
        return torch.float32
    raise TypeError(f"float_type must be np.float32 or np.float64, got {float_type!r}")


def suffix(dtype: torch.dtype) -> str:
    if dtype == torch.float64:
        return "f64"
    if dtype == torch.float32:
        return "f32"
    raise TypeError(f"unsupported dtype {dtype}")


def require_device_tensor(t, dtype, name: str):
    """Type checks mirroring what numba would reject at dispatch time."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a device array (torch.Tensor on the GPU), got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise FusGpuError(f"{name}: tensor is on {t.device}; the operators only run on the GPU (no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"{name}: array must be C-contiguous")
    return t


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr():
    """The caller's current HIP stream (torch's), as the C ABI's ``void* stream``.  The raw getters cost
    ~0.3 us; ``torch.cuda.current_stream()`` builds a Stream object and re-validates the device on every
    call (~3 us of a ~10 us launch from Python: tools/prof_host.py)."""
    if _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_info(device: int = 0):
    lib = load()
    name = C.create_string_buffer(256)
    cu, hbm, lds = C.c_int(0), C.c_int64(0), C.c_int(0)
    check(lib.fus_device_info(device, name, C.byref(cu), C.byref(hbm), C.byref(lds)), "fus_device_info")
    return {"name": name.value.decode(), "compute_units": cu.value, "hbm_bytes": hbm.value, "lds_bytes_per_cu": lds.value}


def set_tuning(key: int, value: int):
    check(load().fus_set_tuning(key, value), "fus_set_tuning")


def get_tuning(key: int) -> int:
    return load().fus_get_tuning(key)
