"""The placement of cell batches on the XCDs by the general-G planned stiffness kernels (csrc/stiffness.hpp: ``group_block``), no GPU
needed: a small host program includes the header and writes the map workgroup id -> batch for every grid size 1 .. 2100 and every group
size; checked here:
  * bijection: a permutation of [0, nblocks) for every nblocks and g (a batch run twice or never is a wrong result);
  * grouping: inside the whole super-groups of 8 g batches, the g blocks 8 m + k (m in one aligned run of g) get g consecutive batches,
    and the eight groups of a round tile their super-group in the order of k;
  * tail: blocks at or behind the last whole super-group map to themselves;
  * g = 0 and g = 1 are the natural order;
and the CPU model of the x fetch (tools/model_x_fetch.py), which states the same map in numpy, is pinned at config 3."""
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
GROUPS = [0, 1, 2, 4, 8, 16, 32, 64, 128, 256]

SOURCE = r"""
#include <cstdio>
#include <vector>
#include "stiffness.hpp"
int main() {
  const int groups[] = {%s};
  std::vector<unsigned> out;
  for (int g : groups)
    for (unsigned nblocks = 1; nblocks <= %du; ++nblocks)
      for (unsigned bid = 0; bid < nblocks; ++bid) out.push_back(fus::group_block(bid, nblocks, g));
  return std::fwrite(out.data(), sizeof(unsigned), out.size(), stdout) == out.size() ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{g: (nblocks of every entry, workgroup id of every entry, batch of every entry)}, grid sizes 1 .. NMAX one after the other"""
    if not _have_hipcc:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("placement")
    src, exe = str(d / "placement.hip"), str(d / "placement")
    with open(src, "w") as f:
        f.write(SOURCE % (", ".join(str(g) for g in GROUPS), NMAX))
    r = subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + CSRC, "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode == 0
    nb = np.repeat(np.arange(1, NMAX + 1, dtype=np.int64), np.arange(1, NMAX + 1))
    bid = np.concatenate([np.arange(k, dtype=np.int64) for k in range(1, NMAX + 1)])
    out = np.frombuffer(r.stdout, dtype=np.uint32).astype(np.int64)
    assert out.size == len(GROUPS) * nb.size
    return {g: (nb, bid, out[i * nb.size:(i + 1) * nb.size]) for i, g in enumerate(GROUPS)}


@pytest.mark.parametrize("g", GROUPS)
def test_map_is_a_permutation(maps, g):
    nb, bid, batch = maps[g]
    assert batch.min() >= 0 and (batch < nb).all()
    # sorted by (grid size, batch) the batches of every grid size must read 0, 1, ..., nblocks - 1
    assert (np.sort(nb * 4096 + batch) == nb * 4096 + bid).all()


@pytest.mark.parametrize("g", [0, 1])
def test_natural_order(maps, g):
    nb, bid, batch = maps[g]
    assert (batch == bid).all()


@pytest.mark.parametrize("g", GROUPS[2:])
def test_tail_keeps_its_place(maps, g):
    nb, bid, batch = maps[g]
    full = nb // (8 * g) * (8 * g)
    tail = bid >= full
    assert tail.any() and (batch[tail] == bid[tail]).all()
    # ... and the whole super-groups map onto themselves, one by one
    assert (batch[~tail] // (8 * g) == bid[~tail] // (8 * g)).all()
    # a group size far above the grid: the natural order
    small = nb < 8 * g
    assert (batch[small] == bid[small]).all()


@pytest.mark.parametrize("g", GROUPS[2:])
def test_groups_of_g_consecutive_batches(maps, g):
    nb, bid, batch = maps[g]
    full = nb // (8 * g) * (8 * g)
    inside = bid < full
    m, k = bid >> 3, bid & 7
    # block 8 m + k, m = j g + i (i < g): batch number i of group k of super-group j
    expect = (m // g) * 8 * g + k * g + m % g
    assert (batch[inside] == expect[inside]).all()
    # said without the formula: the next block of the same XCD label takes the next batch, except across the end of an aligned run
    nxt = inside & (m % g != g - 1)
    idx = np.flatnonzero(nxt)
    assert (bid[idx + 8] == bid[idx] + 8).all() and (nb[idx + 8] == nb[idx]).all()
    assert (batch[idx + 8] == batch[idx] + 1).all()


@pytest.mark.parametrize("g", GROUPS)
def test_numpy_statement_of_the_map_agrees(maps, g):
    """tools/model_x_fetch.py restates group_block for arrays: the model speaks about the map the kernels use"""
    import model_x_fetch

    nb, bid, batch = maps[g]
    for nblocks in (1, 7, 16, 17, 255, 256, 257, 2047, 2048, 2049, NMAX):
        sel = nb == nblocks
        assert (model_x_fetch.group_block(bid[sel], nblocks, g) == batch[sel]).all(), nblocks


def test_model_of_the_x_fetch_at_config_3():
    """P = 4, 54^3 cells, fp64, 128-byte lines.  Natural order: no line is reused in an L2 within 16 batches of an XCD, 181.1 MB per launch
    = 1.585 touches per dof x 1.40 lines per 16 dofs touched x 81.7 MB; g = 16 with a window of 48 batches: 114.3 MB."""
    import model_x_fetch

    r16 = model_x_fetch.model(4, 54, [1], window=16)
    r48 = model_x_fetch.model(4, 54, [1, 16], window=48)
    assert r16["nbatch"] == 15747 and r16["cells_per_batch"] == 10
    assert abs(r16["touches_per_dof"] - 1.585) < 5e-4 and abs(r16["lines_per_16_dofs"] - 1.40) < 5e-3
    assert abs(r16["floor_mb"] - 81.7) < 0.05
    assert abs(r16["mb"][1] - 181.1) < 0.1
    assert abs(r48["mb"][16] - 114.3) < 0.1
    assert r48["mb"][16] < r48["mb"][1] <= r16["mb"][1]
