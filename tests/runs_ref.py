"""Reference of Runs (a plane as run-length records) for the tests: numpy only, no product code.

Semantics (include/infur_hip.h), applied literally:

* a run is a maximal sequence of equal values within one row; it never continues into the next row;
* runs are numbered from 0 in raster order of their first pixel;
* ``flags & SKIP``: runs whose value equals ``skip_value`` are neither emitted nor counted;
* a record is (START = y*w + x of the first pixel, END = one past the last pixel, VALUE zero-extended);
* ``row_start[y]`` is the number of emitted runs that start before row y, ``row_start[h]`` = n.
"""
import numpy as np

SKIP = 1
START, END, VALUE, WORDS = 0, 1, 2, 3


def encode(plane, flags=0, skip_value=0):
    """plane [h, w] of u8 or u32 -> (runs u32 [n, 3], row_start u32 [h + 1], n)"""
    plane = np.asarray(plane)
    assert plane.ndim == 2 and plane.dtype in (np.uint8, np.uint32)
    h, w = plane.shape
    if h * w == 0:
        return np.zeros((0, WORDS), np.uint32), np.zeros(h + 1, np.uint32), 0
    brk = np.ones((h, w), bool)  # x == 0, or the value differs from the left neighbour's
    brk[:, 1:] = plane[:, 1:] != plane[:, :-1]
    start = np.flatnonzero(brk.ravel())
    end = np.append(start[1:], h * w)  # a run ends where the next one begins: rows end in a break, the plane at h*w
    value = plane.ravel()[start].astype(np.uint32)
    if flags & SKIP:
        keep = value != np.uint32(skip_value)
        start, end, value = start[keep], end[keep], value[keep]
    runs = np.stack([start.astype(np.uint32), end.astype(np.uint32), value], axis=1) if len(start) else np.zeros((0, WORDS), np.uint32)
    row_start = np.searchsorted(start, np.arange(h + 1, dtype=np.int64) * w, side="left").astype(np.uint32)
    return runs, row_start, len(start)


def decode(runs, n, h, w, fill, dtype):
    """the dense [h, w] plane of the first min(n, len(runs)) records, `fill` where no record covers a pixel; a plain loop"""
    out = np.full(h * w, fill, dtype)
    for s, e, v in np.asarray(runs)[:n].tolist():
        out[s:e] = v
    return out.reshape(h, w)


def check_invariants(runs, row_start, n, h, w, skipping):
    """what every encoding satisfies: records in range, within one row, START strictly ascending and not overlapping, a monotone
    row index with row_start[h] = n that brackets each row's records; without skip the records tile every row"""
    runs = np.asarray(runs).astype(np.int64)
    assert runs.shape == (n, WORDS) and row_start.shape == (h + 1,)
    s, e = runs[:, START], runs[:, END]
    assert (s < e).all() and (e <= h * w).all()
    if n:
        assert (s // w == (e - 1) // w).all()
        assert (s[1:] >= e[:-1]).all()  # strictly ascending, and no overlap
    rs = row_start.astype(np.int64)
    assert rs[0] == 0 and rs[h] == n and (np.diff(rs) >= 0).all()
    for y in range(h):
        rows = s[rs[y]:rs[y + 1]] // w
        assert (rows == y).all()
    if not skipping and h * w:
        assert s[0] == 0 and e[-1] == h * w and (s[1:] == e[:-1]).all()
        assert (runs[1:, VALUE][s[1:] % w != 0] != runs[:-1, VALUE][s[1:] % w != 0]).all()  # maximal


# ---------------------------------------------------------------- u32 planes: class planes mapped through a table
def u32_table(seed=0):
    """256 distinct u32 values that include 0xFFFFFFFF, 0 and values above 2^24"""
    rng = np.random.default_rng(1000 + seed)
    t = rng.choice(np.arange(1 << 24, 1 << 32, 65537, dtype=np.int64), 256, replace=False).astype(np.uint32)
    t[0], t[1], t[3] = 0xFFFFFFFF, 0, 7
    return t


def as_u32(klass, seed=0):
    return u32_table(seed)[klass]
