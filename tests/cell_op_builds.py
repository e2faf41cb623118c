"""The build matrix of the mass, column and gradient cell kernels: one record per instantiation that the library compiles of

    gradient_plan_geom_kernel  <T, P, CPB, PADLDS, ONEACC, ORDERED, RUNS>   csrc/gradient_geom.hpp   80
    stiffness_col_kernel       <T, P, CPB>                                  csrc/stiffness.hpp       40
    mass_plan_kernel           <T, EPT, EXCL>                               csrc/mass.hpp            36
    mass_kernel                <T, I>                                       csrc/mass.hpp             4

160 in all.  ``template_key`` maps a record onto the tuple that tests/test_cell_model64.py parses from the demangled kernel names of a
device-only compile, by restating the dispatch: ``default_cells_per_block(P, 256 | 128)``, the EPT ladder of ``launch_mass_plan``, the
``total < 0x7fffffff`` split of ``launch_mass`` and ``gradient_single_accumulator<T, P>()``.  The shapes that tests/test_cell_op_builds_gpu.py
launches are here too, so that what they promise (block counts, buckets, ragged batches) is checked without a GPU.  ``POINT_KERNELS``
names the degree list of each point kernel's own GPU test.  No GPU and no torch here."""

import collections

DTYPES = ("f64", "f32")
CTYPE = {"f64": "double", "f32": "float"}
COUNTS = {"gradient_plan_geom_kernel": 80, "stiffness_col_kernel": 40, "mass_plan_kernel": 36, "mass_kernel": 4}
DEGREES = tuple(range(1, 11))

# ``flags``: what steers the dispatch besides the type and the degree, by name
#   gradient   ordered, runs                       (P)
#   col        target: 256 (TUNE_STIFFNESS_VARIANT 0) or 128 (1)   (P)
#   mass_plan  shapes: the (N, epb) pairs the case launches -- all of one bucket of the EPT ladder --, excl
#   mass       total: entries N x nent of the launch
Build = collections.namedtuple("Build", "family dtype P flags")
KERNEL = {"gradient": "gradient_plan_geom_kernel", "col": "stiffness_col_kernel", "mass_plan": "mass_plan_kernel", "mass": "mass_kernel"}


# ---- the dispatch, restated ------------------------------------------------------------------------------------------------------------
def default_cells_per_block(P, target_threads):  # csrc/stiffness.hpp
    return max(target_threads // ((P + 1) ** 2), 1)


def cells_per_batch(P):  # csrc/plan.hpp
    return default_cells_per_block(P, 256)


def col_block_threads(P, cpb):  # csrc/stiffness.hpp: the workgroup is rounded up to whole waves
    return -(-cpb * (P + 1) ** 2 // 64) * 64


EPT_LADDER = (1, 2, 3, 4, 5, 6, 8, 11, 16)  # csrc/mass.hpp: launch_mass_plan
PLAN_MAX_ENTRIES = 4096


def mass_plan_ept(N, epb):
    """(entries per thread asked for, the compiled EPT that serves it)."""
    ept = (N * epb + 255) // 256
    return ept, next(e for e in EPT_LADDER if ept <= e)


def entities_per_batch(N):  # csrc/fus_gpu.hip: fus_plan_entities_per_batch (N = 64, the facet of P = 7, is taken for a cell of P = 3)
    for P in DEGREES:
        if (P + 1) ** 3 == N:
            return cells_per_batch(P)
    return max(1280 // N, 1)


def mass_index_type(total):  # csrc/mass.hpp: launch_mass
    return "unsigned int" if total < 0x7FFFFFFF else "long"


def gradient_single_accumulator(dtype, P):  # csrc/gradient_geom.hpp
    return dtype == "f32" or P in (4, 6, 7, 10)


def remap_block(bid, nblocks):  # csrc/stiffness.hpp, xcd_remap = 1
    per, rem = nblocks >> 3, nblocks & 7
    xcd, idx = bid & 7, bid >> 3
    return xcd * per + min(xcd, rem) + idx


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------
# stiffness_col_kernel, per (P, target): the smallest perturbed box with at least 9 workgroups whose number has the residue mod 8
# assigned to the case -- the residues cycle through 1, 3, 6, 2, 7, 5, 4 down this table, so both sides of ``xcd < rem`` in
# remap_block are taken with every rem -- and whose cell count is no multiple of CPB (where CPB > 1: P >= 8 at 128 threads has CPB = 1)
COL_SHAPES = {(1, 256): (19, 9, 3), (2, 256): (19, 5, 3), (3, 256): (7, 6, 5), (4, 256): (13, 7, 1), (5, 256): (11, 3, 3),
              (6, 256): (31, 2, 1), (7, 256): (5, 3, 3), (8, 256): (5, 5, 1), (9, 256): (7, 3, 1), (10, 256): (3, 3, 3),
              (1, 128): (29, 5, 2), (2, 128): (11, 6, 3), (3, 128): (7, 7, 2), (4, 128): (7, 4, 2), (5, 128): (5, 5, 1),
              (6, 128): (7, 3, 1), (7, 128): (3, 3, 3), (8, 128): (5, 2, 1), (9, 128): (5, 3, 1), (10, 128): (13, 1, 1)}

# mass_plan_kernel through the C ABI, per bucket of the ladder two (entity, degree, epb, box): the first at the bucket's lowest ept,
# the second at its largest N x epb.  "cell": N = (P + 1)^3, "facet": the boundary facets of the box, N = (P + 1)^2.  Every box gives
# more than 2 epb entities, not a multiple of epb: at least three batches, the last one ragged.  EPT 1 and 16 cannot be
# reached from Python (fus_plan_entities_per_batch gives 2 .. 11): M = 256 exactly is N = 8 with epb = 32, M = 4096 is N = 64 with epb = 64
MassShape = collections.namedtuple("MassShape", "entity P epb box")
MASS_PLAN_SHAPES = {
    1: (MassShape("facet", 1, 3, (2, 1, 1)), MassShape("cell", 1, 32, (5, 4, 4))),          # M = 12, 256
    2: (MassShape("cell", 2, 10, (3, 3, 3)), MassShape("cell", 3, 8, (5, 2, 2))),           # M = 270, 512
    3: (MassShape("cell", 2, 19, (7, 3, 2)), MassShape("cell", 3, 12, (5, 3, 2))),          # M = 513, 768
    4: (MassShape("facet", 2, 86, (6, 6, 6)), MassShape("cell", 3, 16, (7, 3, 2))),         # M = 774, 1024
    5: (MassShape("facet", 4, 41, (4, 4, 4)), MassShape("cell", 3, 20, (7, 7, 1))),         # M = 1025, 1280
    6: (MassShape("cell", 2, 48, (5, 5, 4)), MassShape("cell", 3, 24, (5, 4, 3))),          # M = 1296, 1536
    8: (MassShape("cell", 6, 5, (13, 1, 1)), MassShape("cell", 7, 4, (5, 2, 1))),           # M = 1715 (ept 7), 2048
    11: (MassShape("cell", 8, 3, (7, 1, 1)), MassShape("cell", 3, 44, (5, 5, 4))),          # M = 2187 (ept 9), 2816
    16: (MassShape("cell", 9, 3, (7, 1, 1)), MassShape("cell", 3, 64, (6, 5, 5))),          # M = 3000 (ept 12), 4096
}


def mass_shape_N(s):
    return (s.P + 1) ** (3 if s.entity == "cell" else 2)


def mass_shape_entities(s):
    a, b, c = s.box
    return a * b * c if s.entity == "cell" else 2 * (a * b + b * c + c * a)


# mass_plan_kernel from Python (``mass_operator(..., atomic=True)``: the float-atomic batch plan): per degree the smallest box of a few
# tried whose cells hold the 2^15 entries from which the route is taken, with a ragged last batch; facets: a k x k x 1 box
MASS_MIN_ENTRIES = 1 << 15
MASS_CELL_BOXES = {1: (17, 17, 15), 2: (11, 11, 11), 3: (9, 9, 7), 4: (7, 7, 6), 5: (6, 6, 5), 6: (6, 4, 4), 7: (5, 5, 3), 8: (7, 7, 1),
                   9: (7, 5, 1), 10: (3, 3, 3)}
MASS_CELL_EPT = dict(zip(DEGREES, (2, 3, 4, 5, 6, 8, 8, 11, 8, 11)))  # ceil(N cells_per_batch(P) / 256) on the ladder (P = 10: 2662 entries)


def mass_facet_box(P):
    k = 1
    while (2 * k * k + 4 * k) * (P + 1) ** 2 < MASS_MIN_ENTRIES:
        k += 1
    return (k, k, 1)


# mass_kernel: the grid is capped at 256 x 64 workgroups of 256 threads; beyond that many entries a thread takes a second trip
MASS_GRID_ENTRIES = 256 * 64 * 256
MASS_SECOND_TRIP = dict(N=8, nent=MASS_GRID_ENTRIES // 8 + 37, ndofs=50021)
MASS_BIG = dict(N=2048, nent=1 << 20, ndofs=(1 << 20) - 3)  # 2^31 entries, the smallest size that takes the 64-bit build


def _matrix():
    out = []
    for d in DTYPES:
        out += [Build("gradient", d, P, (("ordered", o), ("runs", r))) for P in DEGREES for o in (False, True) for r in (False, True)]
        out += [Build("col", d, P, (("target", t),)) for P in DEGREES for t in (256, 128)]
        out += [Build("mass_plan", d, None, (("shapes", tuple((mass_shape_N(s), s.epb) for s in MASS_PLAN_SHAPES[e])), ("excl", x)))
                for e in EPT_LADDER for x in (False, True)]
        out += [Build("mass", d, None, (("total", t),)) for t in (MASS_SECOND_TRIP["N"] * MASS_SECOND_TRIP["nent"], MASS_BIG["N"] * MASS_BIG["nent"])]
    return out


MATRIX = _matrix()


def template_key(b):
    """(kernel, type, the template arguments behind the type as the demangled name lists them)."""
    f = dict(b.flags)
    if b.family == "gradient":
        args = (b.P, cells_per_batch(b.P), True, gradient_single_accumulator(b.dtype, b.P), f["ordered"], f["runs"])
    elif b.family == "col":
        args = (b.P, default_cells_per_block(b.P, f["target"]))
    elif b.family == "mass_plan":
        buckets = {mass_plan_ept(N, epb)[1] for N, epb in f["shapes"]}
        assert len(buckets) == 1, f"the shapes of one case fall into the buckets {sorted(buckets)}"
        args = (buckets.pop(), f["excl"])
    else:
        args = (mass_index_type(f["total"]),)
    return (KERNEL[b.family], CTYPE[b.dtype], args)


def case_id(b):
    f = dict(b.flags)
    if b.family == "gradient":
        return f"gradient-P{b.P}-{b.dtype}-" + ("ordered" if f["ordered"] else "natural") + ("-runs" if f["runs"] else "-lists")
    if b.family == "col":
        return f"col-P{b.P}-{b.dtype}-cpb{f['target']}"
    if b.family == "mass_plan":
        return f"mass_plan-ept{template_key(b)[2][0]}-{b.dtype}" + ("-excl" if f["excl"] else "-atomic")
    return f"mass-{b.dtype}-" + ("i64" if template_key(b)[2][0] == "long" else "u32")


def of_family(family):
    return [b for b in MATRIX if b.family == family]


# the degree lists of the point kernels' own GPU tests, by (test module, constant): tests/test_cell_model64.py compares each with the
# 20 compiled (T, P) pairs of the kernel
POINT_KERNELS = {"probe_eval_kernel": ("test_sensors_gpu", "DEGREES"), "point_source_kernel": ("test_point_sources_gpu", "DEGREES"),
                 "point_source_wave_kernel": ("test_waveform_sources_gpu", "DEGREES")}
