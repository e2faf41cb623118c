"""The build matrix of the streaming (elementwise) vector kernels: one record per instantiation that the library compiles of

    relax_stage_kernel       <T, NR, W, NT, PERDOF>          csrc/relaxation.hpp        96
    ew_kernel                <T, Op, USE_A, USE_B, VEC, NT>  csrc/vecops.hpp            72
    field_accumulate_kernel  <T, H, W, NT>                   csrc/field_monitor.hpp     60
    mass_gather_kernel       <T, NT, DENSE, R, STATIC>       csrc/mass_gather.hpp       48
    bioheat_stage_kernel     <T, W, NT, LAST>                csrc/bioheat.hpp           24
    muladd_kernel            <T, VEC, NT>                    csrc/vecops.hpp            12
    rk4_stage_kernel         <T, W, NT>                      csrc/rk4.hpp               12
    rk4_stage_nl2_kernel     <T, NT>                         csrc/westervelt.hpp         6
    sponge_terms_kernel      <T, NT>                         csrc/sponge.hpp             6
    rk4_stage_nl_kernel      <T>                             csrc/westervelt.hpp         2

338 in all.  ``template_key`` maps a record onto the tuple that tests/test_stream_builds.py parses from the demangled kernel names of a
device-only compile; ``steer`` gives the run-time settings that make the launcher choose that build (tests/test_stream_builds_gpu.py
applies them); ``vector_stream``, ``aligned16`` and ``stream_blocks`` restate the host rules of csrc/stream_shape.hpp, and ``chosen``
feeds a case's settings through them.  No GPU and no torch here."""

import collections

KERNELS = ("relax_stage_kernel", "ew_kernel", "field_accumulate_kernel", "mass_gather_kernel", "bioheat_stage_kernel", "muladd_kernel",
           "rk4_stage_kernel", "rk4_stage_nl2_kernel", "sponge_terms_kernel", "rk4_stage_nl_kernel")
COUNTS = dict(zip(KERNELS, (96, 72, 60, 48, 24, 12, 12, 6, 6, 2)))
DTYPES = ("f64", "f32")
CTYPE = {"f64": "double", "f32": "float"}
ITEMSIZE = {"f64": 8, "f32": 4}
# ew_kernel's operations: name -> (functor, USE_A, USE_B) (csrc/fus_gpu.hip)
EW_OPS = {"axpy": ("OpAxpy", True, True), "scale": ("OpScale", True, False), "copy": ("OpCopy", True, False), "fill": ("OpFill", False, False),
          "divide": ("OpDiv", True, True), "square": ("OpSquare", True, False)}

# ``flags``: the kernel's own template arguments besides the type, the width and NT, by name (None where the kernel has none of that
# name).  ``W``: dofs per thread (1: the scalar build); kernels without a width (nl, nl2, sponge, the gather) carry 1.
Build = collections.namedtuple("Build", "kernel dtype W NT flags")


def full_width(kernel, dtype, flags=()):
    """Dofs per thread of the wide build: one 16-byte access per array; LAST of an fp32 bioheat field takes 2 (csrc/bioheat.hpp)."""
    if kernel in ("rk4_stage_nl2_kernel", "sponge_terms_kernel", "rk4_stage_nl_kernel", "mass_gather_kernel"):
        return 1
    if kernel == "bioheat_stage_kernel" and dtype == "f32" and dict(flags).get("LAST"):
        return 2
    return 16 // ITEMSIZE[dtype]


def _matrix():
    out = []
    for d in DTYPES:
        widths = lambda k, f=(): (1, full_width(k, d, f))  # noqa: E731
        out += [Build("relax_stage_kernel", d, w, nt, (("NR", nr), ("PERDOF", p)))
                for nr in (1, 2, 3, 4) for w in widths("relax_stage_kernel") for nt in (0, 1, 2) for p in (False, True)]
        out += [Build("ew_kernel", d, w, nt, (("op", op),)) for op in EW_OPS for w in widths("ew_kernel") for nt in (0, 1, 2)]
        out += [Build("field_accumulate_kernel", d, w, nt, (("H", h),)) for h in range(5) for w in widths("field_accumulate_kernel") for nt in (0, 1, 2)]
        out += [Build("mass_gather_kernel", d, 1, nt, (("DENSE", dense), ("R", r), ("STATIC", st)))
                for nt in (0, 1) for dense in (False, True) for r in (1, 2, 4) for st in (False, True)]
        out += [Build("bioheat_stage_kernel", d, w, nt, (("LAST", last),))
                for last in (False, True) for w in widths("bioheat_stage_kernel", (("LAST", last),)) for nt in (0, 1, 2)]
        out += [Build(k, d, w, nt, ()) for k in ("muladd_kernel", "rk4_stage_kernel") for w in widths(k) for nt in (0, 1, 2)]
        out += [Build(k, d, 1, nt, ()) for k in ("rk4_stage_nl2_kernel", "sponge_terms_kernel") for nt in (0, 1, 2)]
        out.append(Build("rk4_stage_nl_kernel", d, 1, 0, ()))
    return out


MATRIX = _matrix()


def template_key(b):
    """(kernel, type, the template arguments behind the type as the demangled name lists them)."""
    f = dict(b.flags)
    if b.kernel == "relax_stage_kernel":
        args = (f["NR"], b.W, b.NT, f["PERDOF"])
    elif b.kernel == "ew_kernel":
        functor, use_a, use_b = EW_OPS[f["op"]]
        args = (functor, use_a, use_b, b.W > 1, b.NT)
    elif b.kernel == "field_accumulate_kernel":
        args = (f["H"], b.W, b.NT)
    elif b.kernel == "mass_gather_kernel":
        args = (b.NT, f["DENSE"], f["R"], f["STATIC"])
    elif b.kernel == "bioheat_stage_kernel":
        args = (b.W, b.NT, f["LAST"])
    elif b.kernel == "muladd_kernel":
        args = (b.W > 1, b.NT)
    elif b.kernel == "rk4_stage_kernel":
        args = (b.W, b.NT)
    elif b.kernel == "rk4_stage_nl_kernel":
        args = ()
    else:
        args = (b.NT,)
    return (b.kernel, CTYPE[b.dtype], args)


def case_id(b):
    f = "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in b.flags)
    return f"{b.kernel[:-7]}-{b.dtype}" + (f"-{f}" if f else "") + f"-W{b.W}-NT{b.NT}"


def steer(b):
    """The run-time settings under which the launcher of ``b.kernel`` picks build ``b``:

    offset        every operand starts this many elements into a 256-byte-aligned allocation: 0 (16-byte accesses allowed) or 1
    odd_stride    relax and the monitor: whether the row stride of the packed arrays is odd (rows that do not start 16-byte aligned)
    mode          ``TUNE_VECTOR_STREAM``: 0 never / 2 always loads and stores / 4 always stores only; the gather streams only under
                  NT = 1, so mode 2 for NT = 1 and mode 0 for NT = 0
    mass_variant  the gather: ``TUNE_MASS_VARIANT`` = rows per thread 1 / 2 / 4
    and the kernel's flags as they are (H, LAST, NR, PERDOF, DENSE, STATIC, op)."""
    f = dict(b.flags)
    wide = b.W > 1
    s = dict(offset=0 if wide or full_width(b.kernel, b.dtype, b.flags) == 1 else 1, mode={0: 0, 1: 2, 2: 4}[b.NT])
    if b.kernel in ("relax_stage_kernel", "field_accumulate_kernel"):
        s["odd_stride"] = not wide
    if b.kernel == "mass_gather_kernel":
        s["mass_variant"] = f["R"]
    s.update(f)
    s.pop("R", None)
    return s


# ---- csrc/stream_shape.hpp, restated ---------------------------------------------------------------------------------------------------
STREAM_BYTES = 24 << 20
STREAM_GRID_CAP, STAGE_GRID_CAP = 2048, 4096
LAUNCH_DOFS = 1 << 27


def vector_stream(operand_bytes, mode=1):
    """NT of a launch on operands of ``operand_bytes`` under ``TUNE_VECTOR_STREAM`` = ``mode``."""
    on = mode in (2, 4) or (mode in (1, 3) and operand_bytes > STREAM_BYTES)
    return 0 if not on else (2 if mode >= 3 else 1)


def aligned16(addresses):
    """Do all of these addresses allow 16-byte accesses?  None (an operand that is switched off) does not count."""
    bits = 0
    for a in addresses:
        bits |= a or 0
    return bits & 15 == 0


def stream_blocks(length, width, cap):
    nblocks = ((length + width - 1) // width + 255) // 256
    return min(nblocks, cap)


def grid_cap(kernel):
    return STAGE_GRID_CAP if kernel.startswith("rk4_stage") else STREAM_GRID_CAP


def chosen(b, settings, n=1027):
    """(W, NT) that the launcher's rules give for build ``b``'s kernel and type under ``settings`` on ``n`` elements: operands at
    ``offset`` elements into allocations at multiples of 256 bytes."""
    size = ITEMSIZE[b.dtype]
    f = dict(b.flags)
    addresses = [256 * k + settings["offset"] * size for k in range(1, 4)]
    ok = aligned16(addresses)
    if b.kernel == "relax_stage_kernel":  # aligned16(bases) && stride % W == 0
        ok = ok and not settings["odd_stride"]
    elif b.kernel == "field_accumulate_kernel":  # ... && (H == 0 || (hstride & 1) == 0)
        ok = ok and (f["H"] == 0 or not settings["odd_stride"])
    width = full_width(b.kernel, b.dtype, b.flags)
    nt = vector_stream(n * size, settings["mode"])
    if b.kernel == "sponge_terms_kernel":
        nt = vector_stream(n * (4 + 2 * size), settings["mode"])
    if b.kernel == "mass_gather_kernel":  # flag_dispatch(vector_stream(...) == 1)
        nt = int(nt == 1)
    if b.kernel == "rk4_stage_nl_kernel":
        nt = 0
    return (width if ok or width == 1 else 1, nt)


# ---- the sizes -------------------------------------------------------------------------------------------------------------------------
def sweep_size(b):
    """Elements at which the grid is at its cap and a few threads take a second iteration of the grid-stride loop: cap x 256 x W +
    777 W + 1 -- three whole workgroups and nine lanes, and one element over a multiple of W.  The gather sweeps rows: see
    ``GATHER_ROWS``."""
    return grid_cap(b.kernel) * 256 * b.W + 777 * b.W + 1


def second_sweep_threads(b):
    """Threads whose grid-stride loop takes a second iteration at ``sweep_size(b)`` (counting whole groups of W for the wide builds)."""
    groups = sweep_size(b) // b.W if b.W > 1 else sweep_size(b)
    return groups - grid_cap(b.kernel) * 256


def gather_rows(r):
    """Touched dofs of the gather's sweep case: 57 row blocks of 256 R (the last one partly live), dealt to the 8 XCDs in chunks of 8:
    every XCD's chunk holds a live workgroup (the eighth: block 56) and 7 of the 64 workgroups return at ``b >= nkb``."""
    return 56 * 256 * r + 131
