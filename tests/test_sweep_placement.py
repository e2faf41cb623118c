"""The sweep direction of the general-G planned stiffness kernels (csrc/stiffness.hpp: ``mirror_block``, ``place_grouped``, the flag bit
``kPlaceReverse`` of the kernels' ``xcd_remap`` argument; knob ``FUS_TUNE_PLAN_SWEEP``), no GPU needed:
  * a small host program includes the header and writes the map workgroup id -> batch for every grid size 1 .. 2100 and g in {0, 1, 2, 16,
    32, 256}, with and without the flag: with it the map is a permutation of [0, nblocks) and equals nblocks - 1 - the unflagged map,
    without it it is ``group_block`` exactly;
  * tests/host/plan_sweep_check.cpp: the parity bit of the plan registry (0, 1, 0, ... per workspace, reset by a rebuild, forgotten by a
    release) and the byte rule of auto (csrc/plan_sweep.hpp), built with the host compiler and run;
  * the LRU model of the memory-side cache (tools/model_g_residency.py) on a hand-checked case and pinned at config 3."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "fenicsx-fus-gpu_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

_have_hipcc = shutil.which("hipcc") is not None or os.path.exists(HIPCC)

NMAX = 2100
GROUPS = [0, 1, 2, 16, 32, 256]

# per g and grid size: group_block, place_grouped without the flag, place_grouped with it; then the value of the flag
SOURCE = r"""
#include <cstdio>
#include <vector>
#include "stiffness.hpp"
int main() {
  const int groups[] = {%s};
  std::vector<unsigned> out;
  for (int g : groups)
    for (unsigned nblocks = 1; nblocks <= %du; ++nblocks) {
      for (unsigned bid = 0; bid < nblocks; ++bid) out.push_back(fus::group_block(bid, nblocks, g));
      for (unsigned bid = 0; bid < nblocks; ++bid) out.push_back(fus::place_grouped(bid, nblocks, g));
      for (unsigned bid = 0; bid < nblocks; ++bid) out.push_back(fus::place_grouped(bid, nblocks, g | fus::kPlaceReverse));
    }
  out.push_back((unsigned)fus::kPlaceReverse);
  out.push_back(fus::mirror_block(3u, 10u, false));
  out.push_back(fus::mirror_block(3u, 10u, true));
  return std::fwrite(out.data(), sizeof(unsigned), out.size(), stdout) == out.size() ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """({g: (nblocks of every entry, workgroup id, group_block, unflagged map, flagged map)}, the three trailing words)"""
    if not _have_hipcc:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("sweep")
    src, exe = str(d / "sweep.hip"), str(d / "sweep")
    with open(src, "w") as f:
        f.write(SOURCE % (", ".join(str(g) for g in GROUPS), NMAX))
    r = subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + CSRC, "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode == 0
    sizes = np.arange(1, NMAX + 1, dtype=np.int64)
    nb = np.repeat(sizes, sizes)
    bid = np.concatenate([np.arange(k, dtype=np.int64) for k in sizes])
    out = np.frombuffer(r.stdout, dtype=np.uint32).astype(np.int64)
    assert out.size == len(GROUPS) * 3 * nb.size + 3
    start = np.concatenate([[0], np.cumsum(3 * sizes)[:-1]])  # where a grid size's three runs begin, within one g

    def pick(block, which):
        return np.concatenate([block[s + which * k:s + (which + 1) * k] for s, k in zip(start, sizes)])

    res = {}
    for i, g in enumerate(GROUPS):
        block = out[i * 3 * nb.size:(i + 1) * 3 * nb.size]
        res[g] = (nb, bid, pick(block, 0), pick(block, 1), pick(block, 2))
    return res, out[-3:]


def test_flag_bit_and_mirror(maps):
    _, tail = maps
    assert list(tail) == [1 << 16, 3, 6]


@pytest.mark.parametrize("g", GROUPS)
def test_without_the_flag_the_map_is_group_block(maps, g):
    nb, bid, grouped, plain, _ = maps[0][g]
    assert (plain == grouped).all()
    if g < 2:
        assert (plain == bid).all()


@pytest.mark.parametrize("g", GROUPS)
def test_flagged_map_is_the_mirrored_permutation(maps, g):
    nb, bid, grouped, _, flagged = maps[0][g]
    assert flagged.min() >= 0 and (flagged < nb).all()
    # sorted by (grid size, batch) the batches of every grid size must read 0, 1, ..., nblocks - 1
    assert (np.sort(nb * 4096 + flagged) == nb * 4096 + bid).all()
    assert (flagged == nb - 1 - grouped).all()
    # the part-filled last batch (and with it the tail behind the last whole super-group) is now run by the first workgroups
    assert (flagged[bid == 0] == (nb - 1 - grouped)[bid == 0]).all()
    small = nb < 8 * max(g, 1)
    assert (flagged[small] == nb[small] - 1 - bid[small]).all()


def test_parity_and_byte_rule_host_program(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "plan_sweep_check")
    src = os.path.join(ROOT, "tests", "host", "plan_sweep_check.cpp")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PLAN_SWEEP_OK" in r.stdout, r.stdout + r.stderr


def test_byte_rule_is_the_roofline_formula():
    """csrc/plan_sweep.hpp restates benchlib/roofline.py's bytes per cell (the host program pins 8044 and the threshold in C++); here the
    Python side of the same numbers, which tests/test_sweep_gpu.py uses to say that its meshes are below the cache."""
    from benchlib.roofline import stiffness_bytes_per_cell

    assert stiffness_bytes_per_cell(4, 8) == 8044 and stiffness_bytes_per_cell(2, 4) == 6 * 27 * 4 + 4 * 27 + 3 * 4 * 8 + 4
    assert stiffness_bytes_per_cell(4, 8) * 33370 <= 256 << 20 < stiffness_bytes_per_cell(4, 8) * 33371
    assert stiffness_bytes_per_cell(4, 8) * 54**3 == 1266640416


def test_lru_model_by_hand():
    """Six batches of 10 bytes of G and 2 of everything else, a cache of 36 bytes = three batches: after 0 .. 5 it holds 3, 4, 5."""
    import model_g_residency as m

    g, other = np.full(6, 10), np.full(6, 2)
    up = np.arange(6)
    assert m.lru_hits(g, other, up, up, 36) == 0  # the cyclic sweep evicts every batch before its turn comes again
    assert m.lru_hits(g, other, up, up[::-1], 36) == 30  # 5, 4, 3 hit; 2, 1, 0 were evicted
    assert m.lru_hits(g, other, up, up, 72) == 60 and m.lru_hits(g, other, up, up[::-1], 72) == 60  # everything fits: either order hits
    assert m.lru_hits(g, other, up, up[::-1], 11) == 0  # not even one batch fits
    uneven = np.array([10, 10, 10, 10, 10, 4])  # a part-filled last batch
    assert m.lru_hits(uneven, other, up, up[::-1], 36) == 24  # 5 (6 bytes), 4, 3 fit in 30 <= 36; 2 would make 42


def test_lru_model_at_config_3():
    """P = 4, 54^3 cells, fp64, g = 32, 256 MiB: a launch moves 1324.3 MB in the model's count (944.8 MB of it G; 15747 batches of 84.1 kB on
    average), so 3120 batches = 187.2 MB of G (19.8 % of G, 14.1 % of the launch) survive to a downward launch, nothing to an upward one.  At 30^3
    cells (the step-0 probe's size: 225.4 MB) everything is resident in either direction."""
    import model_g_residency as m

    r = m.model(4, 54)
    assert r["nbatch"] == 15747 and r["cells_per_batch"] == 10 and r["g_bytes"] == 54**3 * 6000
    assert abs(r["launch_bytes"] / 1e6 - 1324.3) < 0.1
    assert r["up_up"] == 0
    assert abs(r["up_down"] / 1e6 - 187.2) < 0.1
    assert 0.19 < r["up_down"] / r["g_bytes"] < 0.21 and 0.13 < r["up_down"] / r["launch_bytes"] < 0.15
    # natural order (g = 0): the same front, 191.5 MB (the placement inside a window of 256 batches moves the figure by a few MB)
    g, other, info = m.footprint(4, 54)
    up = np.arange(info["nbatch"])
    assert abs(m.lru_hits(g, other, up, up[::-1]) / 1e6 - 191.5) < 0.1 and m.lru_hits(g, other, up, up) == 0
    s = m.model(4, 30)
    assert s["launch_bytes"] < m.CACHE and s["up_up"] == s["up_down"] == s["g_bytes"] == 30**3 * 6000
