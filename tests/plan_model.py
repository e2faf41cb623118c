"""An index model of the two plans the device builds: the batch plan (csrc/plan.hpp, built by csrc/plan_build.hpp) and the transposed
gather plan with its static companion (header comment of csrc/mass_gather.hpp).  numpy only: no torch, no GPU.

The model restates the LAYOUTS and what the builders promise to write, from the layout comments -- ``np.unique``, ``np.searchsorted``
and a stable ``argsort`` where the kernels sort bitonically or by radix.  Everything here is integer data with one right answer, so the
tests that use it (tests/test_plan_model.py on the CPU, tests/test_plan_builders_gpu.py against the device) compare bytes, never with
a tolerance.

Every plan comes with an IMAGE of its workspace and a MASK of the same length:
    mask == DEFINED      the byte has one right value (the image holds it),
    mask == UNSPECIFIED  the builder writes the byte, the layout does not say what (it is never compared),
    mask == UNTOUCHED    the builder must leave the byte alone (alignment gaps, the tail of a ragged batch, a region the call
                         does not fill): it keeps whatever the buffer held.
"""
import numpy as np

DEFINED, UNSPECIFIED, UNTOUCHED = 1, 2, 0

PLAN_MAGIC = 0x46555350314C414E  # "FUSP1LAN"
PLAN_MAX_RUNS = 128
PLAN_MAX_ENTRIES = 4096
PLAN_HEADER_BYTES = 256
PLAN_HEADER_WORDS = 12  # int64 words the builder writes: 0 .. 9 the header proper, 10 / 11 its scratch
SORT_SIZES = (256, 512, 1024, 2048, 4096)

GATHER_MAGIC = 0x4655534D47415431  # "FUSMGAT1"
GATHER_HEADER_BYTES = 256
GATHER_HEADER_FIELDS = ("magic", "nent", "N", "nrows", "dense", "nblocks", "bytes", "max_len", "off_rows", "off_len", "off_base", "off_entries")
GATHER_BLOCK = 256
GATHER_MAX_LEN = 255
STATIC_MAX_SPAN = 65535


def align256(v):
    return (v + 255) // 256 * 256


def plan_row_len(N):
    """n if N = n^3 (a cell plan), 0 otherwise; plan_row_len(1) == 1"""
    n = 1
    while n * n * n < N:
        n += 1
    return n if n * n * n == N else 0


def next_pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def cells_per_batch(P):
    """batch size of a cell plan of degree P: as many cells as give 256 columns, at least one"""
    return max(1, 256 // ((P + 1) ** 2))


def sort_size(M):
    """the build of the sort kernel a batch of M entries takes (launch_plan_build_generic), None if no plan holds it"""
    if M < 1 or M > PLAN_MAX_ENTRIES:
        return None
    return 256 if M <= 256 else 512 if M <= 512 else 1024 if M <= 1024 else 2048 if M <= 2048 else 4096


# ---- batch plan -------------------------------------------------------------------------------------------------------------------

def batch_layout(N, epb, nent):
    """Region offsets of a batch plan: {name: byte offset}, plus ``size`` {name: bytes in use}, nbatch, M, row_len, excl_words, bytes.
    Every region starts on a 256-byte boundary; rowbase and runs_c exist for N = n^3 only; excl is last."""
    nbatch, M, n = -(-nent // epb), epb * N, plan_row_len(N)
    words = (M + 31) // 32
    sizes = [("nu", nbatch * 4), ("udofs", nbatch * M * 4), ("runs", nbatch * 2 * PLAN_MAX_RUNS * 4), ("slot", nbatch * M * 2), ("order", nent * 4)]
    if n > 0:
        sizes += [("rowbase", nbatch * (M // n) * 2), ("runs_c", nbatch * 2 * PLAN_MAX_RUNS * 4)]
    sizes.append(("excl", nbatch * words * 4))
    lay, off = {"nbatch": nbatch, "M": M, "row_len": n, "excl_words": words, "size": dict(sizes)}, PLAN_HEADER_BYTES
    for name, size in sizes:
        lay[name] = off
        off += align256(size)
    lay["bytes"] = off
    return lay


def batch_counts(dofmap, epb, order=None):
    """(nu, nr) of every batch, int64[nbatch] each: the distinct dofs of its valid entries and their maximal stretches of consecutive
    integers.  Vectorised over the full batches (a plan of hundreds of thousands of batches is counted in one sort)."""
    dm = np.asarray(dofmap, dtype=np.int64)
    if order is not None:
        dm = dm[np.asarray(order)]
    nent, N = dm.shape
    full = nent // epb

    def count(rows):
        s = np.sort(rows, axis=1)
        step = np.diff(s, axis=1)
        return 1 + (step != 0).sum(axis=1), 1 + (step > 1).sum(axis=1)

    nu, nr = count(dm[:full * epb].reshape(full, epb * N)) if full else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    if nent > full * epb:
        tu, tr = count(dm[full * epb:].reshape(1, -1))
        nu, nr = np.concatenate([nu, tu]), np.concatenate([nr, tr])
    return nu, nr


class Plan(dict):
    """the fields of a modelled plan, by item or by attribute"""
    __getattr__ = dict.__getitem__


def _put(image, mask, off, arr, state=DEFINED):
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    image[off:off + raw.size] = raw
    mask[off:off + raw.size] = state


def batch_plan(dofmap, epb, order=None, allow_runs=True, fill=0xA5):
    """The batch plan of ``dofmap[nent, N]`` with ``epb`` entities per batch, as csrc/plan.hpp lays it out.

    Per batch b (entities b * epb ... of ``dofmap``, or of ``dofmap[order]``; ``valid`` = its entries, fewer in a ragged last batch):
    ``u`` the sorted distinct dofs, ``nr`` its maximal stretches of consecutive integers, ``use_runs = allow_runs and nr <= 128 and
    2 nr < nu``.  Fields: ``layout``, ``header`` int64[12], ``nu`` (packed words), ``nu_count``, ``nr``, ``use_runs``, ``udofs``
    [nbatch, M], ``runs`` [nbatch, 256], ``slot`` [nbatch, M] and ``rowbase`` [nbatch, M / n] (the tail of a ragged batch holds
    ``fill``), ``runs_c`` [nbatch, 2 run_stride], ``order``; ``image`` / ``mask``: the workspace, byte for byte."""
    dm_in = np.ascontiguousarray(dofmap, dtype=np.int32)
    nent, N = dm_in.shape
    M = epb * N
    assert sort_size(M) is not None, f"no plan holds batches of {M} entries"
    lay = batch_layout(N, epb, nent)
    nbatch, n = lay["nbatch"], lay["row_len"]
    image = np.full(lay["bytes"], fill, np.uint8)
    mask = np.zeros(lay["bytes"], np.uint8)
    p = Plan(layout=lay, N=N, epb=epb, nent=nent, nbatch=nbatch, M=M, row_len=n, ordered=order is not None, image=image, mask=mask)
    if nent == 0:  # the builder returns before it writes anything
        p.update(header=None, nu=np.zeros(0, np.int32), nu_count=np.zeros(0, np.int64), nr=np.zeros(0, np.int64), use_runs=np.zeros(0, bool),
                 u=[], run_stride=PLAN_MAX_RUNS, rows_consecutive=0)
        return p
    dm = dm_in if order is None else dm_in[np.asarray(order)]
    fill16, fill32 = np.uint16(fill * 0x0101), np.uint32(fill * 0x01010101)
    nu = np.zeros(nbatch, np.int32)
    udofs = np.zeros((nbatch, M), np.int32)
    runs = np.zeros((nbatch, 2 * PLAN_MAX_RUNS), np.int32)
    slot = np.full((nbatch, M), fill16, np.uint16)
    rowbase = np.full((nbatch, M // n), fill16, np.uint16) if n else None
    nus, nrs, tables, us = np.zeros(nbatch, np.int64), np.zeros(nbatch, np.int64), np.zeros(nbatch, bool), []
    for b in range(nbatch):
        ent = dm[b * epb:(b + 1) * epb].reshape(-1).astype(np.int64)
        valid = ent.size
        u = np.unique(ent)
        starts = np.concatenate([[0], np.nonzero(np.diff(u) != 1)[0] + 1])  # slot of the first dof of each run
        nr_b = starts.size
        table = bool(allow_runs) and nr_b <= PLAN_MAX_RUNS and 2 * nr_b < u.size
        nus[b], nrs[b], tables[b] = u.size, nr_b, table
        us.append(u)
        nu[b] = u.size | ((nr_b if table else 0) << 16)
        udofs[b, :u.size] = u
        udofs[b, u.size:] = u[0]
        if table:
            runs[b, 0:2 * nr_b:2] = u[starts]
            runs[b, 1:2 * nr_b:2] = starts
        s = np.searchsorted(u, ent)
        slot[b, :valid] = s
        if n:
            rowbase[b, :valid // n] = s[::n]
    rows = dm.reshape(nent, N // n, n).astype(np.int64) if n else None
    broken = int((rows != rows[:, :, :1] + np.arange(n)).any()) if n else 0
    most = int(np.where(tables, nrs, PLAN_MAX_RUNS).max()) if n else 0
    stride = next_pow2(min(max(most, 1), PLAN_MAX_RUNS)) if n else PLAN_MAX_RUNS
    header = np.array([PLAN_MAGIC, N, epb, nent, nbatch, M, int(order is not None), int(tables.sum()), int(n > 0 and not broken), stride,
                       broken, most], np.int64)
    _put(image, mask, 0, header)
    _put(image, mask, lay["nu"], nu)
    _put(image, mask, lay["udofs"], udofs)
    _put(image, mask, lay["runs"], runs)
    valid_last = (nent - (nbatch - 1) * epb) * N
    defined = np.ones((nbatch, M), bool)
    defined[-1, valid_last:] = False
    _put(image, mask, lay["slot"], slot)
    mask[lay["slot"]:lay["slot"] + 2 * nbatch * M] = np.repeat(defined.reshape(-1), 2)
    if order is not None:
        _put(image, mask, lay["order"], np.asarray(order, dtype=np.int32))
    runs_c = None
    if n:
        _put(image, mask, lay["rowbase"], rowbase)
        mask[lay["rowbase"]:lay["rowbase"] + 2 * nbatch * (M // n)] = np.repeat(defined[:, ::n].reshape(-1), 2)
        runs_c = np.ascontiguousarray(runs[:, :2 * stride])
        _put(image, mask, lay["runs_c"], runs_c)
    p.update(header=header, nu=nu, nu_count=nus, nr=nrs, use_runs=tables, u=us, udofs=udofs, runs=runs, slot=slot, rowbase=rowbase, runs_c=runs_c,
             run_stride=stride, rows_consecutive=int(header[8]), order=None if order is None else np.asarray(order, dtype=np.int32), fill32=fill32)
    return p


def exclusive_marks(plan, ndofs, external_use):
    """fus_plan_mark_exclusive on a modelled plan: (``use`` after the call, the ``excl`` words uint32[nbatch, words]).  ``use`` comes in
    as what else touches each dof and gains one per (batch, distinct dof) with 0 <= dof < ndofs; bit s of batch b is set iff s < nu_b,
    the dof is in range and its count is exactly one.  Every word of the region is written.  Also records the region in the plan's
    image and mask."""
    use = np.array(external_use, dtype=np.int32)
    assert use.shape == (ndofs,)
    for u in plan.u:
        inside = u[(u >= 0) & (u < ndofs)]
        use[inside] += 1  # the dofs of one batch are distinct
    excl = np.zeros((plan.nbatch, plan.layout["excl_words"]), np.uint32)
    for b, u in enumerate(plan.u):
        ok = (u >= 0) & (u < ndofs)
        ok[ok] = use[u[ok]] == 1
        s = np.nonzero(ok)[0]
        np.bitwise_or.at(excl[b], s // 32, (np.uint32(1) << (s % 32).astype(np.uint32)))
    if plan.nbatch:
        _put(plan.image, plan.mask, plan.layout["excl"], excl)
    return use, excl


# ---- transposed gather plan -------------------------------------------------------------------------------------------------------

def gather_layout(nent, N, ndofs):
    """the four region offsets and the size of a gather plan: rows int32[maxrows], len uint8[maxrows], base int32[maxblocks + 1],
    entries int32[nent N], maxrows = min(nent N, ndofs)"""
    total = nent * N
    maxrows = min(total, ndofs)
    maxblocks = -(-maxrows // GATHER_BLOCK)
    lay = {"off_rows": GATHER_HEADER_BYTES}
    lay["off_len"] = lay["off_rows"] + align256(maxrows * 4)
    lay["off_base"] = lay["off_len"] + align256(maxrows)
    lay["off_entries"] = lay["off_base"] + align256((maxblocks + 1) * 4)
    lay["bytes"] = lay["off_entries"] + align256(total * 4)
    return lay


def gather_plan(dofmap, ndofs, row_set=None, want=0, fill=0xA5):
    """The transposed plan of ``dofmap[nent, N]`` over a dof vector of length ``ndofs``: per touched dof (a ROW, ascending) the ids
    e * N + i of the entries that hold it, sorted by dof, ties ascending.  ``row_set`` (uint8[ndofs]): only the dofs d with
    row_set[d] == want get a row; the entries of the others sit behind the ``used`` ones and are not specified.

    ``bad``: a value outside [0, ndofs), or a (kept) row of more than 255 entries: nothing usable is built, only ``bad`` is set.
    With no row at all (no entries, or a subset that keeps nothing) only the header is written."""
    dm = np.ascontiguousarray(dofmap, dtype=np.int32)
    nent, N = dm.shape
    total = nent * N
    lay = gather_layout(nent, N, ndofs)
    image = np.full(lay["bytes"], fill, np.uint8)
    mask = np.zeros(lay["bytes"], np.uint8)
    p = Plan(layout=lay, nent=nent, N=N, ndofs=ndofs, image=image, mask=mask, bad=False, **lay)
    keys = dm.reshape(-1).astype(np.int64)
    if ((keys < 0) | (keys >= ndofs)).any():
        p["bad"] = True
        return p
    if row_set is not None:
        keys = np.where(np.asarray(row_set)[keys] == want, keys, ndofs)
    entries = np.argsort(keys, kind="stable").astype(np.int32)
    kept = keys[entries] < ndofs
    used = int(kept.sum())
    rows, counts = np.unique(keys[entries][kept], return_counts=True)
    nrows = rows.size
    if nrows and counts.max() > GATHER_MAX_LEN:
        p["bad"] = True
        return p
    nblocks = -(-nrows // GATHER_BLOCK)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    base = np.concatenate([start[:-1][::GATHER_BLOCK], [used]]).astype(np.int32) if nrows else np.zeros(0, np.int32)
    dense = int(nrows == 0 or bool((rows == np.arange(nrows)).all()))
    max_len = int(counts.max()) if nrows else 0
    fields = dict(magic=GATHER_MAGIC, nent=nent, N=N, nrows=nrows, dense=dense, nblocks=nblocks, bytes=lay["bytes"], max_len=max_len,
                  off_rows=lay["off_rows"], off_len=lay["off_len"], off_base=lay["off_base"], off_entries=lay["off_entries"])
    header = np.array([fields[k] for k in GATHER_HEADER_FIELDS], np.int64)
    _put(image, mask, 0, header)
    if nrows:
        _put(image, mask, lay["off_rows"], rows.astype(np.int32), UNSPECIFIED if dense else DEFINED)
        _put(image, mask, lay["off_len"], counts.astype(np.uint8))
        _put(image, mask, lay["off_base"], base)
    if used < total:  # a subset dropped dofs: their row is written behind the kept ones, their entries behind the used ones
        mask[lay["off_rows"] + 4 * nrows:lay["off_rows"] + 4 * nrows + 4] = UNSPECIFIED
        mask[lay["off_entries"] + 4 * used:lay["off_entries"] + 4 * total] = UNSPECIFIED
    _put(image, mask, lay["off_entries"], entries[:used])
    p.update(fields)
    p.update(header=header, rows=rows.astype(np.int32), len=counts.astype(np.uint8), base=base, entries=entries[:used], used=used, total=total)
    return p


def static_layout(nent, N, elem_bytes):
    """the static companion: detJ_sorted T[nent N], ent16 uint16[nent N], ent_base int32[blocks] and one spare word, each region
    256-byte aligned; sized for every entry being a row of its own"""
    total = nent * N
    lay = {"detJ_sorted": 0, "ent16": align256(total * elem_bytes)}
    lay["ent_base"] = lay["ent16"] + align256(total * 2)
    lay["bytes"] = lay["ent_base"] + align256((-(-total // GATHER_BLOCK) + 1) * 4) + 256
    return lay


def static_companion(gather, detJ, fill=0xA5):
    """The static companion of a modelled gather plan for ``detJ[nent, N]`` (float64 or float32): ``detJ_sorted`` = detJ in entry order
    (a bitwise copy), ``ent_base[b]`` the smallest entity among the entries of 256-row block b, ``ent16`` the entity of each entry
    less its block's base; behind the bases one word holds the widest span of a block.  ``too_wide``: a block spans more than 65 535
    entities -- the bases and the span word are written, nothing else."""
    dj = np.ascontiguousarray(detJ)
    elem = dj.dtype.itemsize
    lay = static_layout(gather.nent, gather.N, elem)
    image = np.full(lay["bytes"], fill, np.uint8)
    mask = np.zeros(lay["bytes"], np.uint8)
    p = Plan(layout=lay, image=image, mask=mask, too_wide=False, **lay)
    if gather.nrows == 0:
        return p
    ent = gather.entries.astype(np.int64) // gather.N
    block = np.repeat(np.arange(gather.nblocks), np.diff(gather.base.astype(np.int64)))  # block of each used entry
    lo = np.full(gather.nblocks, np.iinfo(np.int64).max)
    hi = np.zeros(gather.nblocks, np.int64)
    np.minimum.at(lo, block, ent)
    np.maximum.at(hi, block, ent)
    span = int((hi - lo).max())
    ent_base = lo.astype(np.int32)
    _put(image, mask, lay["ent_base"], np.concatenate([ent_base, [np.int32(span)]]).astype(np.int32))
    p.update(ent_base=ent_base, span=span)
    if span > STATIC_MAX_SPAN:
        p["too_wide"] = True
        return p
    detJ_sorted = dj.reshape(-1)[gather.entries]
    ent16 = (ent - lo[block]).astype(np.uint16)
    _put(image, mask, lay["detJ_sorted"], detJ_sorted)
    _put(image, mask, lay["ent16"], ent16)
    p.update(detJ_sorted=detJ_sorted, ent16=ent16)
    return p


# ---- the cases both test files share ----------------------------------------------------------------------------------------------

# (N, epb): M = 256 ... 4096 exactly and one past each power of two; cell (N = n^3) and other plans mixed
DISPATCH_EDGES = [(4, 64), (257, 1), (16, 32), (27, 19), (64, 16), (25, 41), (512, 4), (683, 3), (64, 64)]
PATTERNS = ("structured", "collide", "high")
CELL_DEGREES = tuple(range(1, 11))
ORDERED = [(27, 19), (125, 10)]
RUN_RULE = (16, 32)
GRID_STRIDE_COUNT = (4, 1, 300_000)  # N, epb, nent: more than 262 144 batches
GRID_STRIDE_FINISH_BATCHES = 4100    # N = 8 cells: more than 1 048 576 words of run tables


def three_batches(epb):
    """entities of a plan of three batches, the last one ragged"""
    return 2 * epb + max(1, epb // 3)


def case_shapes():
    """(case name, N, epb) of every batch plan tests/test_plan_builders_gpu.py builds"""
    out = [(f"edge-{N}x{epb}", N, epb) for N, epb in DISPATCH_EDGES]
    out += [(f"P{P}", (P + 1) ** 3, cells_per_batch(P)) for P in CELL_DEGREES]
    out += [(f"ordered-{N}x{epb}", N, epb) for N, epb in ORDERED]
    out += [("run-rule", *RUN_RULE), ("count-loop", *GRID_STRIDE_COUNT[:2]), ("finish-loop", 8, cells_per_batch(1))]
    return out


def face_of(N):
    """what neighbouring entities of the structured pattern share: a face of a cell, a quarter of any other entity (at least one dof)"""
    n = plan_row_len(N)
    return n * n if n > 1 else max(1, N // 4)


def dof_pattern(kind, N, nent, M, seed=0):
    """int32[nent, N].  structured: entity e holds N consecutive dofs and shares ``face_of(N)`` of them with its neighbour; collide:
    the dofs of a batch drawn from a range a fifth of M wide (duplicates inside a batch and inside an entity); high: structured, shifted so that the
    largest dof is 2^31 - 2."""
    if kind == "collide":  # the window moves on by half its width per batch: neighbouring batches share dofs, and each may own some
        width = max(2, M // 5)
        window = (np.arange(nent) // (M // N)) * (width // 2)
        return (np.random.default_rng(seed).integers(0, width, size=(nent, N)) + window[:, None]).astype(np.int32)
    dm = (np.arange(nent, dtype=np.int64) * (N - face_of(N)))[:, None] + np.arange(N, dtype=np.int64)
    if kind == "high":
        dm += (2 ** 31 - 2) - dm.max()
    else:
        assert kind == "structured"
    return dm.astype(np.int32)


def gather_random_dofmap(seed):
    """The dofmaps of tests/test_operators_gpu.py::test_mass_gather_random_dofmaps: any entity size (1 ... 64), dofs repeated inside an
    entity, hot dofs with up to 250 entries next to a range nobody touches.  Returns (rng, N, nent, nd, dofmap int32[nent, N], counts):
    the generator is handed back in the state the construction left it in (the caller draws its vectors from it)."""
    rng = np.random.default_rng(100 + seed)
    N = int(rng.choice([1, 3, 8, 27, 64]))
    nent = int(rng.integers(1, 4000))
    nd = int(rng.integers(5, 20000))
    dm = rng.integers(0, nd, size=(nent, N))
    # a few hot dofs (at most 250 entries each, the plan's limit is 255) and a dead zone nobody touches
    hot = rng.choice(nd, size=min(3, nd), replace=False)
    flat = dm.reshape(-1)
    for h in hot:
        idx = rng.choice(flat.size, size=min(80, flat.size), replace=False)
        flat[idx] = h
    lo = nd // 3
    flat[(flat >= lo) & (flat < lo + nd // 10)] = 0 if seed % 2 else lo  # empties a range of dofs
    counts = np.bincount(flat, minlength=nd)
    if counts.max() > 255:  # keep inside the plan's limit: spread the excess
        for d in np.nonzero(counts > 250)[0]:
            where = np.nonzero(flat == d)[0][250:]
            flat[where] = rng.integers(lo + nd // 10, nd, size=where.size) if lo + nd // 10 < nd else d
        counts = np.bincount(flat, minlength=nd)
    return rng, N, nent, nd, flat.reshape(nent, N).astype(np.int32), counts
