"""Reference of Raster (polygon loops and run-length records filled back into a plane) for the tests: numpy and plain Python only,
no product code.

The rule of include/infur_hip.h, applied literally:

* pixel (x, y) has its centre at (x + 1/2, y + 1/2); a loop record (OFFSET, COUNT, VALUE, START) is a closed polygon of value V;
* a segment a -> b with y_a != y_b crosses the centre line of every row min(y_a, y_b) <= y < max(y_a, y_b) at the CROSSING COLUMN
  c = ceil((num - dy) / (2 dy)), num = 2 x_0 dy + (x_1 - x_0)(2y + 1 - 2 y_0) with the segment oriented so that dy > 0, clamped to
  0 from below; c >= w has no effect; horizontal segments contribute nothing;
* heading north (y_b < y_a) adds +1 to the winding and +V to the value sum of the pixels x >= c of the row, heading south -1, -V;
* after the prefix sum along the row: OUTSIDE (k = 0, S = 0 mod 2^32: fill), PAINTED (k = 1, and S <= 255 on a byte plane: S),
  CONFLICT (anything else: fill);
* a run record (START, END, VALUE) with START < END <= h*w in one row is +1, +V at START and -1, -V at END unless END ends its row.

``raster`` and ``raster_runs`` are that rule with an accumulator and a cumulative sum.  ``brute`` is a second, independent
reference: per pixel and per loop, the crossing number of the ray to the left of the centre in ``fractions.Fraction`` -- no
crossing column, no prefix sum, no integer division.
"""
from fractions import Fraction

import numpy as np

LOOPS, PAINTED, CONFLICT, STATUS, COUNT_WORDS = 0, 1, 2, 3, 4
TRUNCATED, MALFORMED, OUTSIDE = 1, 2, 4
MASK32 = 0xFFFFFFFF


def _resolve(k, s, dtype, fill):
    """winding k and value sum s (int64 arrays [h, w], s before reduction modulo 2^32) -> (plane, painted, conflict)"""
    s = s & MASK32
    painted = k == 1
    if np.dtype(dtype).itemsize == 1:
        painted &= s <= 255
    outside = (k == 0) & (s == 0)
    plane = np.where(painted, s, fill).astype(dtype)
    return plane, int(painted.sum()), int((~painted & ~outside).sum())


def crossings(xa, ya, xb, yb, w):
    """the crossings of the segment a -> b: (rows, columns, sign), without those at or beyond column w"""
    if ya == yb:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    sign = 1 if yb < ya else -1
    (x0, y0), (x1, y1) = ((xb, yb), (xa, ya)) if yb < ya else ((xa, ya), (xb, yb))
    dy = y1 - y0
    ys = np.arange(y0, y1, dtype=np.int64)
    num = 2 * x0 * dy + (x1 - x0) * (2 * ys + 1 - 2 * y0)
    c = np.maximum(-((dy - num) // (2 * dy)), 0)  # ceil((num - dy) / (2 dy))
    keep = c < w
    return ys[keep], c[keep], sign


def raster(loops, vertices, counts, h, w, dtype=np.uint8, fill=0, loops_rows_in=None, vertex_rows_in=None):
    """-> (plane [h, w] of dtype or None when the input is truncated, counts_out u32 [4])"""
    loops, vertices = np.asarray(loops, np.uint32).reshape(-1, 4), np.asarray(vertices, np.uint32)
    lin = len(loops) if loops_rows_in is None else loops_rows_in
    vin = len(vertices) if vertex_rows_in is None else vertex_rows_in
    nl, nv = int(counts[0]), int(counts[1])
    if nl > lin or nv > vin:
        return None, np.array([nl, 0, 0, TRUNCATED], np.uint32)
    k, s = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    status = 0
    for off, cnt, val, _ in loops[:nl].tolist():
        if cnt < 2 or off + cnt > nv:
            status |= MALFORMED
            continue
        ids = vertices[off:off + cnt].tolist()
        pts = []
        for t in ids:
            x, y = t % (w + 1), t // (w + 1)
            if y > h:
                y = h
                status |= OUTSIDE
            pts.append((x, y))
        for (xa, ya), (xb, yb) in zip(pts, pts[1:] + pts[:1]):
            ys, cs, sign = crossings(xa, ya, xb, yb, w)
            np.add.at(k, (ys, cs), sign)
            np.add.at(s, (ys, cs), sign * val)
    plane, painted, conflict = _resolve(np.cumsum(k, axis=1), np.cumsum(s, axis=1), dtype, fill)
    return plane, np.array([nl, painted, conflict, status], np.uint32)


def raster_runs(runs, n, h, w, dtype=np.uint8, fill=0, runs_rows_in=None):
    """-> (plane or None when truncated, counts_out u32 [4])"""
    runs = np.asarray(runs, np.uint32).reshape(-1, 3)
    rin = len(runs) if runs_rows_in is None else runs_rows_in
    if n > rin:
        return None, np.array([n, 0, 0, TRUNCATED], np.uint32)
    k, s = np.zeros(h * w + 1, np.int64), np.zeros(h * w + 1, np.int64)
    status = 0
    for a, b, val in runs[:n].tolist():
        if not (a < b <= h * w and a // w == (b - 1) // w):
            status |= MALFORMED
            continue
        k[a] += 1
        s[a] += val
        if b % w:
            k[b] -= 1
            s[b] -= val
    k, s = k[:-1].reshape(h, w), s[:-1].reshape(h, w)
    plane, painted, conflict = _resolve(np.cumsum(k, axis=1), np.cumsum(s, axis=1), dtype, fill)
    return plane, np.array([n, painted, conflict, status], np.uint32)


def brute(polys, h, w, dtype=np.uint8, fill=0):
    """polys: [(value, [(x, y), ...])].  Per pixel the winding and the value sum from exact crossing numbers -> (plane, painted,
    conflict).  A centre exactly on a segment counts as lying to its right."""
    plane = np.full((h, w), fill, dtype)
    painted = conflict = 0
    byte = np.dtype(dtype).itemsize == 1
    for y in range(h):
        cy = Fraction(2 * y + 1, 2)
        for x in range(w):
            cx = Fraction(2 * x + 1, 2)
            k = s = 0
            for val, pts in polys:
                for (xa, ya), (xb, yb) in zip(pts, pts[1:] + pts[:1]):
                    if ya == yb or not (min(ya, yb) < cy < max(ya, yb)):
                        continue
                    at = xa + Fraction((xb - xa), (yb - ya)) * (cy - ya)
                    if at <= cx:
                        k += 1 if yb < ya else -1
                        s += val if yb < ya else -val
            s &= MASK32
            if k == 1 and (not byte or s <= 255):
                plane[y, x] = s
                painted += 1
            elif k != 0 or s != 0:
                conflict += 1
    return plane, painted, conflict


def loops_of(polys, w):
    """[(value, [(x, y), ...])] -> (loops u32 [n, 4], vertices u32, counts u32 [2]) in Outlines' layout (START = 0)"""
    loops, vertices = [], []
    for val, pts in polys:
        loops.append((len(vertices), len(pts), val, 0))
        vertices += [y * (w + 1) + x for x, y in pts]
    return (np.array(loops, np.uint32).reshape(-1, 4), np.array(vertices, np.uint32), np.array([len(loops), len(vertices)], np.uint32))


def rect(x0, y0, x1, y1):
    """the clockwise (on a y-down screen) rectangle [x0, x1] x [y0, y1]: an outer loop"""
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
