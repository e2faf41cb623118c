"""The build list of the geometry, boundary-facet and halo kernels (tests/small_kernel_builds.py) on the CPU: that it names every
instantiation of the six kernels that the library compiles, each once, and none that it does not (from the kernel names of a device-only
compile: no GPU); that its grid caps are the launchers'; that every sweep size runs the grid-stride loop a second time; and the census:
every kernel of the library belongs to exactly one family whose builds a test module runs one by one."""

import collections
import os
import re
import shutil
import sys

import pytest

import small_kernel_builds as sk
from conftest import ROOT

_NAME = re.compile(r"fus::(" + "|".join(sk.KERNELS) + r")<(double|float)(?:, (\d+))?>\(")
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


def _compiled_names():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as ru

    return list(ru.parse(ru.cached_remarks()))


@needs_hipcc
def test_the_build_list_is_what_the_library_compiles():
    """As tests/test_stream_builds.py does for the streaming kernels: the two sets of keys are equal and neither holds a key twice."""
    compiled = []
    for name in _compiled_names():
        m = _NAME.search(name)
        if m:
            compiled.append((m.group(1), m.group(2), (int(m.group(3)),) if m.group(3) else ()))
    tested = [sk.template_key(b) for b in sk.BUILDS]
    assert len(compiled) == len(set(compiled)) and len(tested) == len(set(tested)), "a key occurs twice"
    missing, unknown = sorted(set(compiled) - set(tested), key=repr), sorted(set(tested) - set(compiled), key=repr)
    assert not missing, f"{len(missing)} compiled instantiations have no record in the build list: {missing}"
    assert not unknown, f"{len(unknown)} records of the build list name no compiled instantiation: {unknown}"
    assert len(compiled) == 16


def test_the_census_rows_have_names_of_their_own():
    ids = [_row_id(r) for r in sk.CENSUS]
    assert len(set(ids)) == len(ids) and "stiffness_plan_kernel" in ids and "rocprim" in ids, ids


def test_the_counts_per_kernel():
    assert len(sk.BUILDS) == len(set(sk.BUILDS)) == 16 and len({sk.case_id(b) for b in sk.BUILDS}) == 16
    assert collections.Counter(b.kernel for b in sk.BUILDS) == {"geometry_kernel": 2, "facet_geometry_kernel": 2, "facet_terms_kernel": 2,
                                                               "facet_source_array_kernel": 2, "facet_source_wave_kernel": 2, "halo_kernel": 6}
    assert {(b.dtype, b.mode) for b in sk.BUILDS if b.kernel == "halo_kernel"} == {(d, m) for d in ("f64", "f32") for m in (0, 1, 2)}
    text = open(os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc", "halo_layout.hpp")).read()
    m = re.search(r"enum HaloMode[^{]*\{([^}]*)\}", text)
    assert m and [w.split("=")[0].strip() for w in m.group(1).split(",") if w.strip()][:3] == list(sk.HALO_MODES)


@pytest.mark.parametrize("kernel", sk.KERNELS)
def test_the_grid_cap_is_the_launchers(kernel):
    """The body of the kernel's launcher clamps ``nblocks`` to the record's cap, launches blocks of 256 and this kernel."""
    header, launcher, cap, _ = sk.KERNELS[kernel]
    text = open(os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc", header)).read()
    body = text[text.index(f"inline hipError_t {launcher}("):]
    body = body[: body.index("\n}\n")]
    (clamp,) = re.findall(r"if \(nblocks > ([\d *]+)\) nblocks = ([\d *]+);", body)
    value = lambda s: eval(s, {"__builtins__": {}})  # noqa: E731  (a product of integer literals)
    assert value(clamp[0]) == value(clamp[1]) == cap
    assert "(total + 255) / 256" in body or "(count + 255) / 256" in body
    assert f"({kernel}<T" in body and "dim3(256)" in body


@pytest.mark.parametrize("b", sk.BUILDS, ids=[sk.case_id(b) for b in sk.BUILDS])
def test_the_sweep_size_takes_a_second_trip(b):
    """The grid is at its cap (which one workgroup fewer than cap x 256 threads' worth of work would not reach) and between 1 and 999
    threads take a second trip: a few workgroups and a partial one."""
    total = sk.sweep_total(b)
    assert sk.blocks(total, b.cap) == b.cap and sk.blocks(b.cap * 256, b.cap) == b.cap and sk.blocks(b.cap * 256 - 256, b.cap) == b.cap - 1
    assert 1 <= sk.second_trip_threads(b) <= 999
    assert total < 2**31 and total * 6 * 8 < 2**31  # the largest output, an fp64 G, is about 200 MB
    if b.kernel.endswith("geometry_kernel"):  # 997 divides neither the stride nor stride / nq: a wrong index in the second trip shows
        stride = b.cap * 256
        assert stride % 997 != 0 and (stride // b.sweep[1]) % 997 != 0 and stride % b.sweep[1] != 0


def _census(names, table):
    """(names per row, names that match no row, names that match more than one)."""
    rows = [[] for _ in table]
    orphans, twice = [], []
    for name in names:
        hit = [i for i, row in enumerate(table) if re.search(row[0], name)]
        for i in hit:
            rows[i].append(name)
        if not hit:
            orphans.append(name)
        elif len(hit) > 1:
            twice.append(name)
    return rows, orphans, twice


@needs_hipcc
def test_every_compiled_kernel_belongs_to_one_family():
    """The census: every kernel name of the device-only compile matches exactly one row, every row has the number of builds it states,
    its test module exists, and the total is 1808.  A kernel added in a new header matches no row and fails here by name."""
    names = _compiled_names()
    rows, orphans, twice = _census(names, sk.CENSUS)
    assert not orphans, f"{len(orphans)} compiled kernels belong to no family of the census (no test module owns them): {orphans[:8]}"
    assert not twice, f"{len(twice)} compiled kernels match more than one row of the census: {twice[:8]}"
    for (pattern, count, module, _), found in zip(sk.CENSUS, rows):
        assert len(found) == count, f"{pattern}: {len(found)} builds compiled, the census states {count}"
        assert os.path.exists(os.path.join(ROOT, "tests", module)), module
    assert len(names) == len(set(names)) == sum(r[1] for r in sk.CENSUS) == sk.TOTAL == 1808
    # the families of the issue's table
    by = {r[0]: r[1] for r in sk.CENSUS}
    assert by[sk._fus(sk._STREAMING)] == 338 and by[sk._fus(sk._BUILDERS)] == 17 and by[sk._fus(sk._SMALL)] == 16 and by[r"\brocprim::"] == 316


def _row_id(row):
    """The first kernel name of the row's pattern, and how many more it holds."""
    names = re.findall(r"\w+(?:_kernel|::)", row[0].replace("\\b", "").replace("fus::", ""))
    return names[0].rstrip(":") + (f"+{len(names) - 1}" if len(names) > 1 else "")


@needs_hipcc
@pytest.mark.parametrize("drop", range(len(sk.CENSUS)), ids=[_row_id(r) for r in sk.CENSUS])
def test_a_missing_row_orphans_its_kernels(drop):
    """Without any one row the census names that row's kernels as orphans, all of them."""
    table = sk.CENSUS[:drop] + sk.CENSUS[drop + 1:]
    _, orphans, twice = _census(_compiled_names(), table)
    assert len(orphans) == sk.CENSUS[drop][1] and not twice
    assert all(re.search(sk.CENSUS[drop][0], n) for n in orphans)
