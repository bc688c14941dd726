"""Column tiling (test infrastructure): a reference comparison at any size from a C12 fixture.

The moist operators are column-local: what they write to a column depends on that column's inputs alone (its area, land and hs
included).  So an n x n input can be assembled from the 144 columns of a 12 x 12 fixture, and what the reference gave for a
source column is what it would give for every copy of it.  At n = 68 that is a comparison with the reference's run in the second
block of a row (blockIdx.x = 1, four of its 64 lanes), which no fixture reaches.

The map is a sequence of random permutations of the 144 source columns laid over the slots, the slots with i >= 64 first: those
(272 at n = 68) hold every source column, every source column occurs n * n // 144 times or once more, and nothing in the
sequence repeats with a period: the copies of one source column are spread over lanes and rows (check_column_map asserts no
self-mapping shift along either axis, and per source column at least half as many distinct lanes and distinct rows as it has
copies), so an indexing mistake that folds columns onto each other, or a stride that is wrong by a row, lands most copies on
columns of another source."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from make_golden_physics import bits, embed as _embed  # noqa: E402,F401  (the suite's one embedding and one bit view)

SRC = 12  # the fixtures' size
LANES = 64  # columns of a row one block takes (i = is + blockIdx.x * 64 + threadIdx.x)


def column_map(n, seed=0):
    """(si, sj), each of shape (n, n): the column (i, j) of the n x n domain is the fixture's column (si[i, j], sj[i, j])."""
    rng = np.random.default_rng(seed)
    count = n * n
    sequence = np.concatenate([rng.permutation(SRC * SRC) for _ in range(-(-count // (SRC * SRC)))])[:count]
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    # the slots of the blocks after the first come first (a stable sort: row by row within each group)
    order = np.argsort(i.ravel() < LANES, kind="stable")
    source = np.empty(count, dtype=np.int64)
    source[order] = sequence
    source = source.reshape(n, n)
    return source // SRC, source % SRC


def check_column_map(cmap, n):
    """What the tests rely on; raises AssertionError."""
    si, sj = cmap
    assert si.shape == sj.shape == (n, n) and si.min() == sj.min() == 0 and si.max() == sj.max() == SRC - 1
    source = si * SRC + sj
    counts = np.bincount(source.ravel(), minlength=SRC * SRC)
    assert counts.min() >= n * n // (SRC * SRC), counts.min()
    if (n - LANES) * n >= SRC * SRC:
        assert len(np.unique(source[LANES:])) == SRC * SRC, "the blocks after the first do not hold every source column"
    # no periodic tiling: no shift along i or j maps the map onto itself, and the copies of every source column are spread
    # over lanes and rows (at most two of them share a lane or a row where there is room for that)
    for p in range(1, n):
        assert not np.array_equal(source[p:], source[:-p]) and not np.array_equal(source[:, p:], source[:, :-p]), p
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for s in range(SRC * SRC):
        at = source == s
        lanes, rows = np.unique(i[at] % LANES), np.unique(j[at])
        need = min(int(counts[s]), min(n, LANES)) // 2
        assert len(lanes) >= max(need, 1) and len(rows) >= max(need, 1), (s, len(lanes), len(rows), int(counts[s]))


def gather(a, cmap):
    """A fixture array whose first two axes are the 12 x 12 columns -> the same on the n x n columns."""
    assert a.shape[:2] == (SRC, SRC), a.shape
    return np.ascontiguousarray(a[cmap[0], cmap[1]])


def gather_all(d, cmap):
    """gather() for every array of a dict that has the fixture's columns as its first two axes; everything else as it is."""
    return {k: gather(v, cmap) if isinstance(v, np.ndarray) and v.shape[:2] == (SRC, SRC) else v for k, v in d.items()}


def embed(a, n, levels=None, fill=np.nan):
    """A compute-domain array (2-D or 3-D) in `fill`-filled storage of the library's shape: halo 3, one row and one column
    more, `levels` levels (by default one more than the array has)."""
    assert a.shape[:2] == (n, n), a.shape
    return _embed(a, n, fill, levels)


def check_copies(tiled, untiled, cmap, what):
    """`tiled`: an output on the n x n columns; `untiled`: the same library's output on the fixture's own 12 x 12 columns.
    Every copy of a source column holds the bits of the first copy, and those are the bits of the untiled run."""
    si, sj = cmap
    n = si.shape[0]
    source = (si * SRC + sj).ravel()
    first = np.full(SRC * SRC, -1)
    first[source[::-1]] = np.arange(n * n)[::-1]  # (the last assignment wins: the lowest slot)
    flat = bits(tiled).reshape((n * n,) + tiled.shape[2:])
    differ = flat != flat[first[source]]
    assert not differ.any(), (what, int(differ.sum()), "values differ between copies of one column; first at slot",
                              tuple(np.argwhere(differ)[0]))
    differ = bits(tiled) != bits(gather(untiled, cmap))
    assert not differ.any(), (what, int(differ.sum()), "values differ from the untiled run; first at", tuple(np.argwhere(differ)[0]))
