"""fus_reduce_terms_* on the GPU (csrc/reduce.hpp through reductions.Reducer): every build -- double and float, the 16-byte and the
scalar access -- at the sizes where the launch changes shape, against exact integer sums, against math.fsum within the bound that
follows from the addition tree (tests/reduce_model.py), with non-finite entries, and bitwise twice."""
import ctypes as C
import math

import numpy as np
import pytest
import reduce_model as rm
from conftest import pkg

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DTYPES = {"f64": (np.float64, 8), "f32": (np.float32, 4)}


def sizes(itemsize):
    """Empty, one entry, one pair, either side of a workgroup, several workgroups with a tail, and past the grid cap: the grid-stride
    loop's second, partial trip (for the scalar build of the offset operands its third or fifth)."""
    return [0, 1, 2, 255, 256, 257, 4099, rm.GRID_CAP * rm.BLOCK * (16 // itemsize) + 997]


CASES = [pytest.param(key, aligned, k, id=f"{key}-{'aligned' if aligned else 'offset'}-n{k}") for key in DTYPES for aligned in (True, False)
         for k in range(8)]
TERM_SETS = ("sum0", "sum0c", "both_x", "x")


@pytest.fixture(scope="module")
def reducer():
    return pkg("reductions").Reducer()


_host = {}


def host_operands(kind, n):
    """Seven host vectors of ``n`` float32 values, made once per (kind, n) and left unchanged.  ``ints``: integers in [-3, 3], so that
    every partial sum of products is an integer below 2^53 and exact whatever the order.  ``decades``: signed values spread over six
    decades with 17-bit mantissas, so that each product of three is exact in double (reduce_model.short_mantissa)."""
    if (kind, n) not in _host:
        rng = np.random.default_rng(n + (17 if kind == "ints" else 0))
        if kind == "ints":
            v = rng.integers(-3, 4, size=(7, n)).astype(np.float32)
        else:
            v = rm.short_mantissa(rng.choice([-1.0, 1.0], size=(7, n)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(7, n)))
        _host[(kind, n)] = v
    return _host[(kind, n)]


def on_device(host, np_dtype, aligned):
    """The rows of ``host`` as device vectors of ``np_dtype``: views from element 0 of their allocation, or from element 1 (not 16-byte
    aligned: the scalar build)."""
    n, off = host.shape[1], 0 if aligned else 1
    out = []
    for row in host:
        buf = torch.zeros(n + off, dtype=torch.float64 if np_dtype == np.float64 else torch.float32, device="cuda")
        buf[off:].copy_(torch.from_numpy(row.astype(np_dtype)))
        view = buf[off:]
        assert (view.data_ptr() % 16 == 0) == aligned or n == 0
        out.append(view)
    return out


def term_arguments(name, v):
    a0, b0, c0, a1, b1, c1, x = v
    return {"sum0": dict(sum0=(a0, b0, None)), "sum0c": dict(sum0=(a0, b0, c0)), "both_x": dict(sum0=(a0, b0, c0), sum1=(a1, b1, None), x=x),
            "x": dict(x=x)}[name]


def model_arguments(name, h):
    a0, b0, c0, a1, b1, _, x = h
    return {"sum0": dict(a0=a0, b0=b0), "sum0c": dict(a0=a0, b0=b0, c0=c0), "both_x": dict(a0=a0, b0=b0, c0=c0, a1=a1, b1=b1, x=x),
            "x": dict(x=x)}[name]


@pytest.mark.parametrize("key, aligned, k", CASES)
def test_exact_integer_sums(reducer, key, aligned, k):
    """Small integers: the result must EQUAL the integer sums; a dropped or doubled entry shows as a wrong integer."""
    np_dtype, itemsize = DTYPES[key]
    n = sizes(itemsize)[k]
    host = host_operands("ints", n)
    dev = on_device(host, np_dtype, aligned)
    for name in TERM_SETS:
        got = reducer.terms(n=n, **term_arguments(name, dev)).tolist()
        sums, _, amax, bad = rm.expected(**model_arguments(name, host))
        assert got == [sums[0], sums[1], amax, float(bad)], (name, n, got)
        if n == 0:
            assert got == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("key, aligned, k", CASES)
def test_rounding_within_the_tree_bound(reducer, key, aligned, k):
    """Values over six decades: |got - exact| <= depth 2^-53 sum|t_i|, depth counted from the launch's shape (reduce_model.depth:
    derived, not measured).  The products are exact in double by construction, so math.fsum is the exact sum correctly rounded."""
    np_dtype, itemsize = DTYPES[key]
    n = sizes(itemsize)[k]
    host = host_operands("decades", n)
    dev = on_device(host, np_dtype, aligned)
    depth = rm.depth(n, itemsize, aligned)
    for name in TERM_SETS:
        got = reducer.terms(n=n, **term_arguments(name, dev)).tolist()
        sums, mags, amax, bad = rm.expected(**model_arguments(name, host))
        for s in range(2):
            err, bound = abs(got[s] - sums[s]), depth * 2.0**-53 * mags[s]
            print(f"{key} {'aligned' if aligned else 'offset'} n={n} {name} sum{s}: error {err:.3e}, bound {bound:.3e} (depth {depth})")
            assert err <= bound, (name, s, got[s], sums[s])
        assert got[2] == amax and got[3] == bad  # comparisons only: bitwise


def test_large_vector_pieces_and_offsets(reducer):
    """One fp32 vector of 2^27 + 1000 entries (512 MB, past kLaunchDofs: two pieces, byte offsets up to 2^29, rows of both pieces in
    one finish launch), aliased as a0 = b0 = x.  Integers in [-3, 3]: the sum of squares is an exact integer."""
    n = rm.LAUNCH_DOFS + 1000
    x = ((torch.arange(n, dtype=torch.int32, device="cuda") * 5) % 7 - 3).to(torch.float32)
    want = int((x.to(torch.int64) ** 2).sum().item())
    got = reducer.terms(sum0=(x, x, None), x=x, n=n).tolist()
    assert got == [float(want), 0.0, 3.0, 0.0]
    x[n - 1] = float("nan")  # the second piece is read, to its last entry
    x[rm.LAUNCH_DOFS - 1] = -50.0
    again = reducer.terms(x=x, n=n).tolist()
    assert again == [0.0, 0.0, 50.0, 1.0]


@pytest.mark.parametrize("key", list(DTYPES))
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
def test_non_finite_entries(reducer, key, aligned):
    """A NaN in the last entry (the scalar tail of the 16-byte build), +Inf in the grid-stride loop's second trip and -Inf in the
    first entry (the misaligned head of the offset operands): three are counted, out[2] is the largest FINITE magnitude, and the sum
    over the same vector is not a number."""
    np_dtype, itemsize = DTYPES[key]
    w = 16 // itemsize
    n = sizes(itemsize)[-1]
    assert n % w == 1  # the last entry is the tail's
    host = host_operands("ints", n)[6:7].copy()
    host[0, n - 1], host[0, rm.GRID_CAP * rm.BLOCK * w + 5], host[0, 0] = np.nan, np.inf, -np.inf
    host[0, 12345] = -7.5
    (x,) = on_device(host, np_dtype, aligned)
    got = reducer.terms(sum0=(x, x, None), x=x, n=n).tolist()
    assert got[2] == 7.5 and got[3] == 3.0 and math.isnan(got[0]) and got[1] == 0.0
    assert reducer.absmax(x, n=n) == (7.5, 3)
    only_bad = torch.full((5,), float("inf"), dtype=x.dtype, device="cuda")
    assert reducer.terms(x=only_bad).tolist() == [0.0, 0.0, 0.0, 5.0]


@pytest.mark.parametrize("key", list(DTYPES))
def test_bitwise_reproducible(reducer, key):
    np_dtype, itemsize = DTYPES[key]
    n = sizes(itemsize)[-1]
    dev = on_device(host_operands("decades", n), np_dtype, True)
    args = term_arguments("both_x", dev)
    first = reducer.terms(n=n, **args).clone()
    second = reducer.terms(n=n, **args).clone()
    reducer._ws.fill_(float("nan"))  # what the workspace holds on entry does not matter
    third = reducer.terms(n=n, **args).clone()
    as_bits = lambda t: t.view(torch.int64).tolist()  # noqa: E731
    assert as_bits(first) == as_bits(second) == as_bits(third)
    out = torch.full((3, 4), -1.0, dtype=torch.float64, device="cuda")  # a row of a caller's series
    assert reducer.terms(n=n, out=out[1], **args) is not None
    assert as_bits(out[1]) == as_bits(first) and out[0].tolist() == [-1.0] * 4 and out[2].tolist() == [-1.0] * 4


def test_dot_and_checks(reducer):
    a = torch.arange(10, dtype=torch.float64, device="cuda")
    w = torch.full((10,), 0.5, dtype=torch.float64, device="cuda")
    assert reducer.dot(a, a) == 285.0 and reducer.dot(a, a, w) == 142.5 and reducer.dot(a, a, w, n=4) == 7.0
    assert reducer.absmax(-a) == (9.0, 0)
    with pytest.raises(TypeError):
        reducer.dot(a, a.to(torch.float32))
    with pytest.raises(pkg("_lib").FusGpuError):
        reducer.dot(a.cpu(), a.cpu())
    with pytest.raises(ValueError):
        reducer.dot(a, a, n=11)
    with pytest.raises(ValueError):
        reducer.terms()


def test_invalid_arguments_launch_nothing():
    lib = pkg("_lib").load()
    out = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(64, dtype=torch.float64, device="cuda")
    a = torch.ones(8, dtype=torch.float64, device="cuda")
    z, p = C.c_void_p(0), lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    fn = lib.fus_reduce_terms_f64
    assert fn(p(a), p(a), z, z, z, z, z, -1, p(out), p(ws), z) == -1
    assert fn(p(a), z, z, z, z, z, z, 8, p(out), p(ws), z) == -1
    assert fn(z, z, z, p(a), z, z, z, 8, p(out), p(ws), z) == -1
    assert fn(p(a), p(a), z, z, z, z, z, 8, z, p(ws), z) == -1
    assert fn(p(a), p(a), z, z, z, z, z, 8, p(out), z, z) == -1
    torch.cuda.synchronize()
    assert out.tolist() == [-1.0] * 4  # nothing ran
    assert fn(p(a), p(a), z, z, z, z, z, 8, p(out), p(ws), z) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [8.0, 0.0, 0.0, 0.0]
