"""The build list of the geometry, boundary-facet and halo kernels: one record per instantiation that the library compiles of

    geometry_kernel            <T>        csrc/geometry.hpp       launch_geometry              2    cap 16384 blocks of 256
    facet_geometry_kernel      <T>        csrc/geometry.hpp       launch_facet_geometry        2    cap 16384
    facet_terms_kernel         <T>        csrc/mass.hpp           launch_facet_terms           2    cap 4096
    facet_source_array_kernel  <T>        csrc/source_array.hpp   launch_facet_source_array    2    cap 4096
    facet_source_wave_kernel   <T>        csrc/source_wave.hpp    launch_facet_source_wave     2    cap 4096
    halo_kernel                <T, MODE>  csrc/halo.hpp           launch_halo                  6    cap 2048    MODE 0 PACK, 1 UNPACK_SET, 2 UNPACK_ADD

16 in all.  Every kernel is one grid-stride loop over ``total`` threads' worth of work: entries (halo), (cell, q) or (facet, q) pairs
(geometry), (facet, local dof) pairs of both sets (the three facet-term kernels).  ``sweep`` is the shape at which the grid is at its cap
and fewer than 1000 threads take a second trip of that loop: (entities, per entity), whose product is the total.  tests/
test_small_kernel_builds.py compares the list with the kernel names of a device-only compile and the caps with the launchers' text;
tests/test_small_kernels_gpu.py runs every record.  No GPU and no torch here."""

import collections

CTYPE = {"f64": "double", "f32": "float"}
HALO_MODES = ("PACK", "UNPACK_SET", "UNPACK_ADD")  # csrc/halo_layout.hpp: HaloMode 0, 1, 2
BLOCK = 256

Build = collections.namedtuple("Build", "kernel dtype mode header launcher cap sweep")

# kernel: (header, launcher, grid cap, sweep shape)
#   geometry          599 298 cells x nq = 7           = 16384 x 256 + 782
#   facet geometry    466 120 facets x nqf = 9         = 16384 x 256 + 776
#   facet terms       41 960 facets (A and B) x N = 25 =  4096 x 256 + 424
#   halo              525 065 entries                  =  2048 x 256 + 777
KERNELS = {
    "geometry_kernel": ("geometry.hpp", "launch_geometry", 16384, (599298, 7)),
    "facet_geometry_kernel": ("geometry.hpp", "launch_facet_geometry", 16384, (466120, 9)),
    "facet_terms_kernel": ("mass.hpp", "launch_facet_terms", 4096, (41960, 25)),
    "facet_source_array_kernel": ("source_array.hpp", "launch_facet_source_array", 4096, (41960, 25)),
    "facet_source_wave_kernel": ("source_wave.hpp", "launch_facet_source_wave", 4096, (41960, 25)),
    "halo_kernel": ("halo.hpp", "launch_halo", 2048, (525065, 1)),
}

BUILDS = [Build(k, d, m, *KERNELS[k]) for k in KERNELS for d in CTYPE for m in (range(3) if k == "halo_kernel" else (None,))]


def template_key(b):
    """(kernel, type, the template arguments behind the type as the demangled name lists them)."""
    return (b.kernel, CTYPE[b.dtype], () if b.mode is None else (b.mode,))


def case_id(b):
    return f"{b.kernel[:-7]}-{b.dtype}" + ("" if b.mode is None else f"-{HALO_MODES[b.mode]}")


def sweep_total(b):
    return b.sweep[0] * b.sweep[1]


def blocks(total, cap):
    """The launchers' grid: one thread per unit of work, at most ``cap`` workgroups of 256."""
    return min((total + BLOCK - 1) // BLOCK, cap)


def second_trip_threads(b):
    """Threads that take a second trip of the grid-stride loop at the sweep size."""
    return sweep_total(b) - blocks(sweep_total(b), b.cap) * BLOCK


def of(kernel, dtype, mode=None):
    (b,) = [b for b in BUILDS if (b.kernel, b.dtype, b.mode) == (kernel, dtype, mode)]
    return b


# ---- the census: every kernel of the library belongs to one family, and every family to a test module --------------------------------
# (pattern that the demangled name must contain, number of builds, the test module that runs every build of it, a note).  The first
# seventeen families are those of the build matrices; the last three are rows of their own for the reason beside them.
_STREAMING = ("relax_stage_kernel|ew_kernel|field_accumulate_kernel|mass_gather_kernel|bioheat_stage_kernel|muladd_kernel|rk4_stage_kernel|"
              "rk4_stage_nl2_kernel|sponge_terms_kernel|rk4_stage_nl_kernel")
_BUILDERS = ("plan_build_kernel|plan_count_runs_kernel|plan_count_uses_kernel|plan_finish_kernel|plan_mark_exclusive_kernel|gather_flag_kernel|"
             "gather_iota_kernel|gather_len_kernel|gather_rows_kernel|gather_static_base_kernel|gather_static_fill_kernel|gather_subset_keys_kernel")
_SMALL = "|".join(KERNELS)


def _fus(names):
    return r"\bfus::(?:" + names + r")[<(]"


CENSUS = [
    (_fus("stiffness_plan_kernel"), 232, "test_cell_builds_gpu.py", ""),
    (_fus("stiffness_plan_rows_kernel"), 14, "test_cell_builds_gpu.py", ""),
    (_fus("stiffness_plan_affine_kernel"), 80, "test_cell_builds_gpu.py", ""),
    (_fus("stiffness_plan_geom_kernel"), 80, "test_cell_builds_gpu.py", ""),
    (_fus("stiffness_plan_geom_nodal_kernel"), 80, "test_nodal_builds_gpu.py", ""),
    (_fus("westervelt_cell_kernel"), 160, "test_cell_builds_gpu.py", ""),
    (_fus("westervelt_cell_geom_kernel"), 160, "test_cell_builds_gpu.py", ""),
    (_fus("westervelt_cell_geom_nodal_kernel"), 80, "test_nodal_builds_gpu.py", ""),
    (_fus("gradient_plan_geom_kernel"), 80, "test_cell_op_builds_gpu.py", ""),
    (_fus("stiffness_col_kernel"), 40, "test_cell_op_builds_gpu.py", ""),
    (_fus("mass_plan_kernel"), 36, "test_cell_op_builds_gpu.py", ""),
    (_fus("mass_kernel"), 4, "test_cell_op_builds_gpu.py", ""),
    (_fus(_STREAMING), 338, "test_stream_builds_gpu.py", "the ten streaming vector kernels of tests/stream_builds.py"),
    (_fus("point_source_kernel"), 20, "test_point_sources_gpu.py", ""),
    (_fus("point_source_wave_kernel"), 20, "test_waveform_sources_gpu.py", ""),
    (_fus("probe_eval_kernel"), 20, "test_sensors_gpu.py", ""),
    (_fus("element_receive_kernel"), 2, "test_receivers_gpu.py", ""),
    (_fus(_BUILDERS), 17, "test_plan_builders_gpu.py", "the plan and gather builders of tests/plan_model.py"),
    (_fus(_SMALL), 16, "test_small_kernels_gpu.py", "the builds of this module"),
    (r"\brocprim::", 316, "test_plan_builders_gpu.py", "library code behind the plan builders' sorts and scans: run through them, not a kernel of this project"),
    (_fus("ipc_send_kernel|ipc_recv_kernel"), 10, "test_halo_gpu.py", "the peer transport: needs two devices that map each other's memory; run by the peer-transport tests"),
    (_fus("stream_signal_kernel|stream_wait_kernel|displaced_signal_kernel"), 3, "test_halo_gpu.py",
     "one-word flag kernels of the communicator's fork and join: one build each, no arithmetic; run by every overlapped halo exchange"),
]
TOTAL = 1808
