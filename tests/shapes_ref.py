"""Reference of Shapes (area, moments, convex hull and minimum rectangle per outline loop, sums per value) for the tests: numpy and
plain Python only, no product code.

It applies the definitions of include/infur_hip.h literally.  For one loop v_0 .. v_{n-1}, with v_n := v_0 and
c_i = x_i y_{i+1} - x_{i+1} y_i:

* the seven measures are sums over i in Python integers, which do not overflow; they are reduced to signed 64-bit words only at the
  end;
* the hull is Andrew's monotone chain over the distinct points, strict (a point on a hull edge is dropped); a kept point is written
  at its first index in the loop, and the kept indices come out ascending: the loop's own order;
* the rectangle is a brute-force search over all hull edges, compared by exact cross-multiplication, ties to the smallest edge.

``emulate`` is the second implementation: the device kernels' lane logic (shapes.hip) -- the strided sums that wrap at 64 bits, the
strided argmin / argmax with their tie order, the register stack over cyclic index ranges, the walk that drops collinear vertices,
the rank of the flag scan, the rectangle's strided edges and butterfly -- which must equal the definitions.
"""
import numpy as np

from simplify_ref import _xy

OFFSET, COUNT, VALUE, START, WORDS = 0, 1, 2, 3, 4
(AREA2, PERIMETER, M10_6, M01_6, M20_12, M02_12, M11_24, HULL_AREA2, RECT_EDGE, RECT_W, RECT_H, RECT_L, SHAPE_WORDS) = range(13)
OUTER, HOLES, LOOP = 8, 9, 10
STATUS_TRUNCATED, STATUS_MALFORMED = 1, 2
M64 = (1 << 64) - 1
POISON32, POISON64 = 0xA5A5A5A5, np.uint64(0xA5A5A5A5A5A5A5A5).astype(np.int64)


def signed64(v):
    """an integer modulo 2^64 as the signed word that holds it"""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def measures(x, y):
    """the seven sums of one loop given as lists x, y, exact"""
    n = len(x)
    s = [0] * 7
    for i in range(n):
        xi, yi, xj, yj = x[i], y[i], x[(i + 1) % n], y[(i + 1) % n]
        c = xi * yj - xj * yi
        s[0] += c
        s[1] += abs(xj - xi) + abs(yj - yi)
        s[2] += c * (xi + xj)
        s[3] += c * (yi + yj)
        s[4] += c * (xi * xi + xi * xj + xj * xj)
        s[5] += c * (yi * yi + yi * yj + yj * yj)
        s[6] += c * (xi * yj + 2 * xi * yi + 2 * xj * yj + xj * yi)
    return s


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_indices(x, y):
    """the indices of the strictly extreme points of one loop, each at its first occurrence, ascending"""
    first = {}
    for i, p in enumerate(zip(x, y)):
        first.setdefault(p, i)
    pts = sorted(first)
    if len(pts) <= 2:
        return sorted(first[p] for p in pts)
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return sorted(first[p] for p in set(lower[:-1] + upper[:-1]))


def shoelace2(hx, hy):
    k = len(hx)
    return sum(hx[j] * hy[(j + 1) % k] - hx[(j + 1) % k] * hy[j] for j in range(k))


def rectangle(hx, hy):
    """(edge, W, H, L) of the smallest rectangle on an edge of the hull given in order; zeros for a single point"""
    k = len(hx)
    best = None
    for j in range(k):
        ex, ey = hx[(j + 1) % k] - hx[j], hy[(j + 1) % k] - hy[j]
        dots = [ex * px + ey * py for px, py in zip(hx, hy)]
        w = max(dots) - min(dots)
        h = max(abs(ex * (py - hy[j]) - ey * (px - hx[j])) for px, py in zip(hx, hy))
        length = ex * ex + ey * ey
        if best is None or w * h * best[3] < best[1] * best[2] * length:
            best = (j, w, h, length)
    return best if best and best[3] else (0, 0, 0, 0)


def loop_shape(x, y, hull_fn=hull_indices):
    """one loop -> (its per-loop record of 12 Python integers, the kept indices)"""
    kept = hull_fn(x, y)
    hx, hy = [x[i] for i in kept], [y[i] for i in kept]
    return measures(x, y) + [shoelace2(hx, hy)] + list(rectangle(hx, hy)), kept


def shapes(loops, vertices, counts, w, rows=0, loops_rows_in=None, vertex_rows_in=None, hull_fn=hull_indices):
    """Outlines' (loops, vertices, counts) of a plane of width w -> (loops_out u32 [n_loops, 4], vertices_out u32 [n_hull],
    shapes i64 [n_loops, 12], values i64 [rows, 12], counts_out u32 [4] = n_loops, n_hull_vertices, status, largest COUNT').
    Truncated input: no loops, no vertices, no records, the per-value table of a plane without loops, counts_out = {counts[0], 0, 1, 0}."""
    assert 0 < w <= 8191
    loops = np.asarray(loops, np.uint32).reshape(-1, WORDS)
    vertices = np.asarray(vertices, np.uint32).reshape(-1)
    lrows = len(loops) if loops_rows_in is None else loops_rows_in
    vrows = len(vertices) if vertex_rows_in is None else vertex_rows_in
    nl, nv = int(counts[0]), int(counts[1])
    values = [[0] * 10 + [-1, 0] for _ in range(rows)]
    best = [None] * rows
    as_values = lambda: np.array([[signed64(v) for v in row] for row in values], np.int64).reshape(rows, SHAPE_WORDS)  # noqa: E731
    if nl > lrows or nv > vrows:
        return (np.zeros((0, WORDS), np.uint32), np.zeros(0, np.uint32), np.zeros((0, SHAPE_WORDS), np.int64), as_values(),
                np.array([nl, 0, STATUS_TRUNCATED, 0], np.uint32))
    keep = np.zeros(nv, bool)
    status = 0
    recs, well = [], []
    for i, (off, cnt, val, _) in enumerate(loops[:nl].tolist()):
        ok = cnt >= 2 and off + cnt <= nv
        well.append(ok)
        if not ok:
            status |= STATUS_MALFORMED
            recs.append([0] * SHAPE_WORDS)
            continue
        x, y = _xy(vertices[off:off + cnt], w)
        rec, kept = loop_shape(x, y, hull_fn)
        recs.append(rec)
        keep[off + np.array(kept, np.int64)] = True
        if val < rows:
            row = values[val]
            for k in range(7):
                row[k] += rec[k]
            if rec[AREA2] > 0:
                row[HULL_AREA2] += rec[HULL_AREA2]
                row[OUTER] += 1
                if best[val] is None or rec[AREA2] > best[val]:
                    best[val], row[LOOP] = rec[AREA2], i
            elif rec[AREA2] < 0:
                row[HOLES] += 1
    rank = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    out = np.zeros((nl, WORDS), np.uint32)
    for i, (off, cnt, val, start) in enumerate(loops[:nl].tolist()):
        out[i] = (rank[min(off, nv)], rank[off + cnt] - rank[off] if well[i] else 0, val, start)
    sh = np.array([[signed64(v) for v in r] for r in recs], np.int64).reshape(nl, SHAPE_WORDS)
    largest = int(out[:, COUNT].max()) if nl else 0
    return out, vertices[:nv][keep].copy(), sh, as_values(), np.array([nl, int(rank[nv]), status, largest], np.uint32)


def hull_xy(loops_out, vertices_out, i, w):
    """the hull of loop i as lists x, y"""
    off, cnt = int(loops_out[i][OFFSET]), int(loops_out[i][COUNT])
    return _xy(vertices_out[off:off + cnt], w)


def check_invariants(loops, vertices, w, loops_out, vertices_out, shapes_out):
    """the facts of the sweep, for well-formed loops of a plane: the kept sequence is a subsequence that is strictly convex with
    the loop's orientation, contains every vertex, and an outer loop starts on its hull"""
    loops = np.asarray(loops, np.uint32).reshape(-1, WORDS)
    for i, (off, cnt, _, _) in enumerate(loops.tolist()):
        x, y = _xy(vertices[off:off + cnt], w)
        hx, hy = hull_xy(loops_out, vertices_out, i, w)
        k = len(hx)
        a2 = int(shapes_out[i][AREA2])
        assert k >= 3 and a2 != 0
        src, at = list(zip(x, y)), 0
        for p in zip(hx, hy):  # a subsequence, each hull vertex once
            at = src.index(p, at) + 1
        assert len(set(zip(hx, hy))) == k
        sgn = 1 if a2 > 0 else -1
        for j in range(k):
            o, a, b = (hx[j], hy[j]), (hx[(j + 1) % k], hy[(j + 1) % k]), (hx[(j + 2) % k], hy[(j + 2) % k])
            assert sgn * _cross(o, a, b) > 0  # strictly convex, in the loop's orientation
            assert all(sgn * _cross(o, a, p) >= 0 for p in src)  # every vertex on the inner side of every hull edge
        if a2 > 0:
            assert (hx[0], hy[0]) == src[0]
        assert abs(int(shapes_out[i][HULL_AREA2])) >= abs(a2) and int(shapes_out[i][HULL_AREA2]) * sgn > 0


# ---------------------------------------------------------------- the kernels' lane logic
LANES = 64
NONE = 0xFFFFFFFF


def _butterfly(vals, better):
    """xor-butterfly over 64 lanes: a lane takes its partner's value when better(partner, own)"""
    v = list(vals)
    step = 32
    while step:
        v = [v[lane ^ step] if better(v[lane ^ step], v[lane]) else v[lane] for lane in range(LANES)]
        step >>= 1
    assert all(t == v[0] for t in v)  # every lane ends with the same answer
    return v[0]


def _wave_sum(vals):
    v = list(vals)
    step = 32
    while step:
        v = [(v[lane] + v[lane ^ step]) & M64 for lane in range(LANES)]
        step >>= 1
    assert all(t == v[0] for t in v)
    return v[0]


def _strided_argmax(fn, lo, hi):
    """every lane walks lo + lane, lo + lane + 64, .. < hi and keeps its first maximum of fn; an idle lane holds (0, 2^32 - 1);
    the larger value wins, the smaller index on a tie"""
    keys = [(0, NONE)] * LANES
    for lane in range(LANES):
        first = True
        for i in range(lo + lane, hi, LANES):
            v = fn(i)
            if first or v > keys[lane][0]:
                keys[lane], first = (v, i), False
    return _butterfly(keys, lambda o, m: o[0] > m[0] or (o[0] == m[0] and o[1] < m[1]))


def hull_loop_lanes(x, y):
    """one loop as the hull kernel computes it -> (the seven measures modulo 2^64, the kept indices ascending)"""
    n = len(x)
    at = lambda k: (x[k - n if k >= n else k], y[k - n if k >= n else k])  # noqa: E731  (k below 2n)
    sums = [[0] * LANES for _ in range(7)]
    lo_key, hi_key = [M64] * LANES, [0] * LANES
    for lane in range(LANES):
        for i in range(lane, n, LANES):
            (xi, yi), (xj, yj) = at(i), at(i + 1)
            c = (xi * yj - xj * yi) & M64
            terms = (c, abs(xj - xi) + abs(yj - yi), c * (xi + xj), c * (yi + yj), c * (xi * xi + xi * xj + xj * xj), c * (yi * yi + yi * yj + yj * yj),
                     c * (xi * yj + 2 * xi * yi + 2 * xj * yj + xj * yi))
            for k in range(7):
                sums[k][lane] = (sums[k][lane] + terms[k]) & M64
            yx = (yi << 14 | xi) << 32
            lo_key[lane], hi_key[lane] = min(lo_key[lane], yx | i), max(hi_key[lane], yx | (NONE - i))
    m = [_wave_sum(s) for s in sums]
    lo = _butterfly(lo_key, lambda o, own: o < own) & NONE
    hi = NONE - (_butterfly(hi_key, lambda o, own: o > own) & NONE)
    keep = [0] * n
    keep[lo] = 1
    if lo != hi:
        keep[hi] = 1
        sgn = -1 if signed64(m[0]) < 0 else 1
        big = hi if hi > lo else hi + n
        stack = [None] * LANES
        stack[0], sp = (big, lo + n), 1
        a, c = lo, big
        while True:
            if c - a < 2:
                if sp == 0:
                    break
                sp -= 1
                a, c = stack[sp]
                continue
            (ax, ay), (cx, cy) = at(a), at(c)
            ex, ey = cx - ax, cy - ay
            best, mid = _strided_argmax(lambda i: max(0, sgn * (ey * (at(i)[0] - ax) - ex * (at(i)[1] - ay))), a + 1, c)
            if best > 0:
                assert sp < LANES and a < mid < c
                keep[mid - n if mid >= n else mid] = 1
                if mid - a >= c - mid:  # the larger half waits, the smaller is next
                    stack[sp], a = (a, mid), mid
                else:
                    stack[sp], c = (mid, c), mid
                sp += 1
                assert sp <= max(2, n).bit_length() + 1
            else:
                c = a
    # the walk from lo that drops a kept vertex collinear with its kept neighbours; flags are read a chunk at a time, before its drops
    turn = lambda p, q, r: (at(q)[0] - at(p)[0]) * (at(r)[1] - at(q)[1]) - (at(q)[1] - at(p)[1]) * (at(r)[0] - at(q)[0])  # noqa: E731
    pos = lambda t: lo + t - n if lo + t >= n else lo + t  # noqa: E731
    c1 = c2 = f0 = f1 = None
    total = 0
    for b in range(0, n, LANES):
        mask = [t for t in range(b, min(b + LANES, n)) if keep[pos(t)]]
        for j, t in enumerate(mask):
            p1 = mask[j - 1] if j >= 1 else c1
            p2 = mask[j - 2] if j >= 2 else (c1 if j == 1 else c2)
            if p1 is not None and p2 is not None and turn(lo + p2, lo + p1, lo + t) == 0:
                keep[pos(p1)] = 0
        if mask:
            if f0 is None:
                f0 = mask[0]
                if len(mask) > 1:
                    f1 = mask[1]
            elif f1 is None:
                f1 = mask[0]
            c2 = mask[-2] if len(mask) >= 2 else c1
            c1 = mask[-1]
            total += len(mask)
    if total >= 3:
        if turn(lo + c2, lo + c1, lo + f0) == 0:
            keep[pos(c1)] = 0
        if turn(lo + c1, lo + f0, lo + f1) == 0:
            keep[pos(f0)] = 0
    return m, [i for i in range(n) if keep[i]]


def _rect_before(a, b):
    """(w, h, l, j) a before b: the smaller w h / l exactly, the smaller j on a tie; j == NONE: no edge yet"""
    if a[3] == NONE or b[3] == NONE:
        return b[3] == NONE and a[3] != NONE
    p, q = a[0] * a[1] * b[2], b[0] * b[1] * a[2]
    assert p < 1 << 128 and q < 1 << 128
    return p < q or (p == q and a[3] < b[3])


def rect_lanes(hx, hy):
    """the rect kernel on one hull -> (HULL_AREA2 modulo 2^64, (edge, W, H, L))"""
    k = len(hx)
    area, best = [0] * LANES, [(0, 0, 0, NONE)] * LANES
    for lane in range(LANES):
        for j in range(lane, k, LANES):
            vx, vy, ux, uy = hx[j], hy[j], hx[(j + 1) % k], hy[(j + 1) % k]
            area[lane] = (area[lane] + vx * uy - ux * vy) & M64
            ex, ey = ux - vx, uy - vy
            dots = [ex * px + ey * py for px, py in zip(hx, hy)]
            far = max(abs(ex * (py - vy) - ey * (px - vx)) for px, py in zip(hx, hy))
            r = (max(dots) - min(dots), far, ex * ex + ey * ey, j)
            assert all(t < 1 << 32 for t in r)
            if _rect_before(r, best[lane]):
                best[lane] = r
    w, h, length, j = _butterfly(best, _rect_before)
    return _wave_sum(area), ((j, w, h, length) if k else (0, 0, 0, 0))


_LANES_SEEN = {}


def emulate(loops, vertices, counts, w, rows=0, loops_rows_in=None, vertex_rows_in=None, loops_rows_out=None, vertex_rows_out=None,
            shape_rows=None, block=1024):
    """the launches of shapes.hip in numpy on buffers of the declared rows -> (loops_out [loops_rows_out, 4], vertices_out
    [vertex_rows_out], shapes [shape_rows, 12], values [rows, 12], counts_out [4]); what a launch leaves alone holds 0xA5 bytes"""
    loops = np.asarray(loops, np.uint32).reshape(-1, WORDS)
    vertices = np.asarray(vertices, np.uint32).reshape(-1)
    lrows = len(loops) if loops_rows_in is None else loops_rows_in
    vrows = len(vertices) if vertex_rows_in is None else vertex_rows_in
    loops, vertices = loops[:lrows], vertices[:vrows]  # no lane reads beyond the declared rows
    c0, c1 = int(counts[0]), int(counts[1])
    truncated = c0 > lrows or c1 > vrows
    nl, nv = (0, 0) if truncated else (c0, c1)
    lro = nl if loops_rows_out is None else loops_rows_out
    sro = nl if shape_rows is None else shape_rows
    keep = np.zeros(vrows + 1, np.uint8)  # (the memsets)
    values = [[0] * SHAPE_WORDS for _ in range(rows)]
    sign = [0] * nl
    sh = np.full((sro, SHAPE_WORDS), POISON64, np.int64)
    # hull: one wave per loop
    for i in range(nl):
        off, cnt, val = int(loops[i, OFFSET]), int(loops[i, COUNT]), int(loops[i, VALUE])
        well = cnt >= 2 and off + cnt <= nv
        m = [0] * 7
        if well:
            x, y = _xy(vertices[off:off + cnt], w)
            key = (tuple(x), tuple(y))
            if key not in _LANES_SEEN:
                _LANES_SEEN[key] = hull_loop_lanes(x, y)
            m, kept = _LANES_SEEN[key]
            keep[off + np.array(kept, np.int64)] = 1
        a2 = signed64(m[0])
        sign[i] = 0 if not well or a2 == 0 else 1 if a2 > 0 else 2
        if i < sro:
            sh[i, :7] = [signed64(v) for v in m]
        if well and val < rows:
            for k in range(7):
                values[val][k] = (values[val][k] + m[k]) & M64
            if a2 > 0:
                values[val][OUTER] += 1
                values[val][LOOP] = max(values[val][LOOP], a2 << 32 | (NONE - i))
            elif a2 < 0:
                values[val][HOLES] += 1
    # sums, partials, rank over the positions 0 .. vrows
    flag = np.zeros(vrows + 1, np.int64)
    flag[:nv] = keep[:nv]
    nb = (vrows + 1 + block - 1) // block
    sums = np.add.reduceat(np.concatenate([flag, np.zeros(nb * block - len(flag), np.int64)]), np.arange(nb) * block)
    base = np.cumsum(sums) - sums
    rank = np.zeros(vrows + 1, np.int64)
    for blk in range(nb):
        f = flag[blk * block:(blk + 1) * block]
        rank[blk * block:blk * block + len(f)] = base[blk] + np.cumsum(f) - f
    n_out = int(sums.sum())
    vro = n_out if vertex_rows_out is None else vertex_rows_out
    vout = np.full(vro, POISON32, np.uint32)
    hull = np.zeros(vrows + 1, np.uint32)
    for p in np.flatnonzero(flag).tolist():
        hull[rank[p]] = vertices[p]
        if rank[p] < vro:
            vout[rank[p]] = vertices[p]
    # rect: one wave per loop
    lout = np.full((lro, WORDS), POISON32, np.uint32)
    bad = largest = 0
    for i in range(nl):
        off, cnt, val, start = (int(t) for t in loops[i])
        well = cnt >= 2 and off + cnt <= nv
        first = int(rank[min(off, nv)])
        k = int(rank[off + cnt]) - first if well else 0
        hx, hy = _xy(hull[first:first + k], w)
        area, rect = rect_lanes(hx, hy)
        bad |= not well
        largest = max(largest, k)
        if i < lro:
            lout[i] = (first, k, val, start)
        if i < sro:
            sh[i, 7:] = [signed64(area)] + list(rect)
        if sign[i] == 1 and val < rows:
            values[val][HULL_AREA2] = (values[val][HULL_AREA2] + area) & M64
    for row in values:  # finish
        row[LOOP] = NONE - (row[LOOP] & NONE) if row[LOOP] else -1
    vals = np.array([[signed64(v) for v in row] for row in values], np.int64).reshape(rows, SHAPE_WORDS)
    return lout, vout, sh, vals, np.array([c0, n_out, (1 if truncated else 0) | (2 if bad else 0), largest], np.uint32)


# ---------------------------------------------------------------- planes and loops for the tests
def disc(r):
    """(x - r - 1)^2 + (y - r - 1)^2 <= r^2 on a (2r + 3)^2 plane, class 1 on class 0"""
    g = np.arange(2 * r + 3) - r - 1
    return (g[None, :] ** 2 + g[:, None] ** 2 <= r * r).astype(np.uint8)


def annulus(r, r_in):
    """a disc with a round hole: the hole's loop does not start on its hull, so its ranges wrap"""
    g = np.arange(2 * r + 3) - r - 1
    d2 = g[None, :] ** 2 + g[:, None] ** 2
    return ((d2 <= r * r) & (d2 > r_in * r_in)).astype(np.uint8)


def letter_c():
    """worked example 1: a 24 x 24 plane, class 1 = [2:22, 2:22] minus [7:17, 7:22]"""
    p = np.zeros((24, 24), np.uint8)
    p[2:22, 2:22] = 1
    p[7:17, 7:22] = 0
    return p


def bar():
    """worked example 2: a 12 x 16 plane, value 2 where |(x - 8) - (y - 6)| <= 1, 1 <= y <= 10 and 1 <= x <= 14"""
    y, x = np.mgrid[0:12, 0:16]
    return (2 * ((np.abs((x - 8) - (y - 6)) <= 1) & (y >= 1) & (y <= 10) & (x >= 1) & (x <= 14))).astype(np.uint8)


def loop_of(points, w, value=1, start=0):
    """hand-made input: one loop through the lattice points [(x, y)] of a plane of width w -> (loops, vertices, counts)"""
    ids = np.array([y * (w + 1) + x for x, y in points], np.uint32)
    return np.array([[0, len(ids), value, start]], np.uint32), ids, np.array([1, len(ids), 0], np.uint32)


def diagonal_staircase(steps, side=8191):
    """a closed staircase of `steps` unit-ish steps along the diagonal of the side x side square and back along its two sides:
    about 2 * steps vertices whose moment sums wrap at 64 bits on the way and fit in the end"""
    at = [side * k // steps for k in range(steps + 1)]
    pts = []
    for k in range(steps):  # (0,0) -> (side, side): right, then down
        pts += [(at[k], at[k]), (at[k + 1], at[k])]
    pts += [(side, side), (0, side)]
    return pts


def polygon_of(n):
    """a loop of exactly n >= 4 vertices: a staircase of n // 2 - 1 steps closed by its two sides; an odd n has one more vertex in
    the middle of the closing side, collinear with its neighbours (no plane makes one: the input is hand-made)"""
    k = n // 2 - 1
    pts = []
    for i in range(k):
        pts += [(i, i), (i + 1, i)]
    pts += [(k, k), (0, k)]
    if n % 2:
        pts.append((0, k // 2))
    assert len(pts) == n and len(set(pts)) == n
    return pts


def pixel_sums(mask):
    """the six identities' right-hand sides from the pixels of a boolean mask, exact: AREA2, M10_6, M01_6, M20_12, M02_12, M11_24"""
    ys, xs = np.nonzero(mask)
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    return [2 * len(xs), 3 * sum(2 * x + 1 for x in xs), 3 * sum(2 * y + 1 for y in ys), 2 * sum(6 * x * x + 6 * x + 2 for x in xs),
            2 * sum(6 * y * y + 6 * y + 2 for y in ys), 6 * sum((2 * x + 1) * (2 * y + 1) for x, y in zip(xs, ys))]
