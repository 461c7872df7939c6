"""Reference of Coverage (shared borders simplified once) for the tests: numpy and plain Python only, no product code.

It restates the contract of include/infur_hip.h sequentially.

* CELLS.  A cell outside the plane, or (under SKIP) equal to skip_value, is *none*: one value, distinct from every plane value.
  Lattice vertex (X, Y) has the cells UL = (X-1, Y-1), UR = (X, Y-1), LL = (X-1, Y), LR = (X, Y); ray N is a border when UL != UR,
  S when LL != LR, W when UL != LL, E when UR != LR.  A JUNCTION is a vertex with three or four border rays.
* AUGMENT.  For every edge v_i -> v_{i+1} of a loop (cyclic): v_i, then the junctions strictly inside the edge in travel order.
  An edge that is not axis-parallel, has no length or has an id outside the lattice makes the loop MALFORMED, as does a record
  with COUNT < 2 or OFFSET + COUNT > n_vertices.
* ARCS.  The augmented loop is cut at its junction vertices; the stretch from one to the next (cyclically; the same vertex twice
  when the loop has one) is an arc, and a loop without a junction is a ring.
* SPLIT(0, k) on an arc u_0 .. u_k is Simplify's with one change: m is the i with maximal D_i and, on ties, the smallest vertex
  id (and, should one id occur twice in a hand-made loop, the first in travel order).  A ring's anchors are A, the vertex with
  the smallest id, and B, which maximises |v - A|^2 (ties: smallest id); SPLIT runs on A..B and B..A.
* OUTPUT.  Simplify's layout; counts_out = {n_loops, n_vertices', n_degenerate, status, n_aug, n_arcs}.

Python integers do not overflow.  ``pairing`` and ``check_invariants`` state what the stage is for: every directed segment of the
output has its reverse in another loop, except the plane's frame.
"""
import functools
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402  (the plane generators)

SKIP = 1
OFFSET, COUNT, VALUE, START, WORDS = 0, 1, 2, 3, 4
COUNT_WORDS = 6
STATUS_TRUNCATED, STATUS_MALFORMED, STATUS_OVERFLOW = 1, 2, 4
MAX_SIDE = 8191
NONE_VALUE = 0xFFFFFFFF
WIDTHS = (63, 64, 65, 127, 129)


def cells(plane, flags=0, skip_value=0):
    """[h + 2, w + 2] int64: the plane with -1 (none) around it and at every skipped pixel; cell (x, y) is at [y + 1, x + 1]"""
    plane = np.asarray(plane)
    assert plane.ndim == 2 and plane.dtype in (np.uint8, np.uint32)
    h, w = plane.shape
    v = np.full((h + 2, w + 2), -1, np.int64)
    v[1:-1, 1:-1] = plane
    if flags & SKIP:
        v[1:-1, 1:-1][plane == skip_value] = -1
    return v


def degrees(plane, flags=0, skip_value=0):
    """-> int [h + 1, w + 1]: the number of border rays of every lattice vertex (0, 2, 3 or 4)"""
    v = cells(plane, flags, skip_value)
    ul, ur, ll, lr = v[:-1, :-1], v[:-1, 1:], v[1:, :-1], v[1:, 1:]
    return (ul != ur).astype(np.int64) + (ll != lr) + (ul != ll) + (ur != lr)


def junctions(plane, flags=0, skip_value=0):
    return degrees(plane, flags, skip_value) >= 3


def augment(ids, junction):
    """one loop's vertex ids -> (augmented ids, junction flags) as lists, or None when an edge is malformed"""
    h1, w1 = junction.shape
    n = len(ids)
    out, flag = [], []
    for i in range(n):
        a, b = int(ids[i]), int(ids[(i + 1) % n])
        if a >= h1 * w1 or b >= h1 * w1:
            return None
        xa, ya, xb, yb = a % w1, a // w1, b % w1, b // w1
        if (xa == xb) == (ya == yb):  # a diagonal, or no length
            return None
        out.append(a)
        flag.append(bool(junction[ya, xa]))
        if ya == yb:
            step = 1 if xb > xa else -1
            inside = [ya * w1 + x for x in range(xa + step, xb, step) if junction[ya, x]]
        else:
            step = 1 if yb > ya else -1
            inside = [y * w1 + xa for y in range(ya + step, yb, step) if junction[y, xa]]
        out += inside
        flag += [True] * len(inside)
    return out, flag


def split(ids, w1, tol16):
    """SPLIT(0, k) on the vertex ids u_0 .. u_k -> the set of kept interior indices"""
    k = len(ids) - 1
    if k < 2:
        return set()
    arr = np.asarray(ids, np.int64)
    x, y = arr % w1, arr // w1
    t2 = tol16 * tol16
    kept = set()
    todo = [(0, k)]
    while todo:
        a, c = todo.pop()
        if c - a < 2:
            continue
        ex, ey = int(x[c] - x[a]), int(y[c] - y[a])
        length = ex * ex + ey * ey
        dx, dy = x[a + 1:c] - x[a], y[a + 1:c] - y[a]
        d = (ex * dy - ey * dx) ** 2 if length else dx * dx + dy * dy  # (below 2^54: int64 holds it)
        dm = int(d.max())
        cand = np.flatnonzero(d == dm)
        m = a + 1 + int(cand[np.argmin(arr[a + 1:c][cand])])  # the smallest id; argmin takes the first of equal ids
        if 256 * dm > t2 * (length or 1):
            kept.add(m)
            todo += [(a, m), (m, c)]
    return kept


def keep_loop(aug, flag, w1, tol16):
    """one augmented loop -> (bool list: kept, the number of arcs: a ring is one)"""
    n = len(aug)
    keep = [False] * n
    heads = [p for p in range(n) if flag[p]]
    if not heads:
        arr = np.asarray(aug, np.int64)
        a = int(np.argmin(arr))
        turned = np.roll(arr, -a)  # travel order from A on: equal ids, which no plane produces, tie to the first
        d = (turned % w1 - arr[a] % w1) ** 2 + (turned // w1 - arr[a] // w1) ** 2
        cand = np.flatnonzero(d == d.max())
        b = (a + int(cand[np.argmin(turned[cand])])) % n
        keep[a] = keep[b] = True
        for s, e in ((a, b), (b, a)):
            length = (e - s) % n or n
            pos = [(s + t) % n for t in range(length + 1)]
            for t in split([aug[p] for p in pos], w1, tol16):
                keep[pos[t]] = True
        return keep, 1
    for j, s in enumerate(heads):
        e = heads[(j + 1) % len(heads)]
        length = (e - s) % n or n
        pos = [(s + t) % n for t in range(length + 1)]
        keep[s] = True
        for t in split([aug[p] for p in pos], w1, tol16):
            keep[pos[t]] = True
    return keep, len(heads)


def coverage(plane, loops, vertices, counts, tol16, flags=0, skip_value=0, loops_rows_in=None, vertex_rows_in=None, aug_rows=0):
    """the plane Outlines was given and its (loops [*, 4], vertices [*], counts [>= 2]) -> (loops_out u32 [n_loops, 4], vertices_out
    u32 [n_vertices'], counts_out u32 [6]).  The rows default to the arrays' lengths; aug_rows = 0 is vertex_rows_in + (h+1)(w+1)."""
    plane = np.asarray(plane)
    h, w = plane.shape
    assert 0 < w <= MAX_SIDE and 0 < h <= MAX_SIDE and 0 <= tol16 <= 65535 and not flags & ~SKIP
    loops = np.asarray(loops, np.uint32).reshape(-1, WORDS)
    vertices = np.asarray(vertices, np.uint32).reshape(-1)
    lrows = len(loops) if loops_rows_in is None else loops_rows_in
    vrows = len(vertices) if vertex_rows_in is None else vertex_rows_in
    arows = aug_rows or vrows + (h + 1) * (w + 1)
    nl, nv = int(counts[0]), int(counts[1])
    none = (np.zeros((0, WORDS), np.uint32), np.zeros(0, np.uint32))
    if nl > lrows or nv > vrows:
        return none + (np.array([nl, 0, 0, STATUS_TRUNCATED, 0, 0], np.uint32),)
    junction = junctions(plane, flags, skip_value)
    w1 = w + 1
    status = 0
    augmented = []
    for off, cnt, _, _ in loops[:nl].tolist():
        res = augment(vertices[off:off + cnt].tolist(), junction) if cnt >= 2 and off + cnt <= nv else None
        if res is None:
            status |= STATUS_MALFORMED
        augmented.append(res)
    n_aug = sum(len(r[0]) for r in augmented if r)
    if n_aug > arows:
        return none + (np.array([nl, 0, 0, STATUS_OVERFLOW, min(n_aug, 0xFFFFFFFF), 0], np.uint32),)
    out = np.zeros((nl, WORDS), np.uint32)
    vout = []
    n_arcs = 0
    for i, ((off, cnt, val, start), res) in enumerate(zip(loops[:nl].tolist(), augmented)):
        at = len(vout)
        if res:
            keep, arcs = keep_loop(res[0], res[1], w1, tol16)
            n_arcs += arcs
            vout += [t for t, k in zip(res[0], keep) if k]
        out[i] = (at, len(vout) - at, val, start)
    n_deg = int((out[:, COUNT] < 3).sum())
    return out, np.array(vout, np.uint32), np.array([nl, len(vout), n_deg, status, n_aug, n_arcs], np.uint32)


# ---------------------------------------------------------------- what the stage guarantees
def segments(loops_out, vertices_out):
    """Counter of the directed segments (p, q) of all loops, with multiplicity"""
    seg = Counter()
    v = np.asarray(vertices_out).tolist()
    for off, cnt, _, _ in np.asarray(loops_out).tolist():
        ids = v[off:off + cnt]
        for p, q in zip(ids, ids[1:] + ids[:1]):
            if p != q:
                seg[(p, q)] += 1
    return seg


def unpaired(loops_out, vertices_out):
    """{(p, q): N(p, q)} for the segments with N = count(p -> q) - count(q -> p) != 0, each pair reported from its positive side"""
    seg = segments(loops_out, vertices_out)
    out = {}
    for (p, q), n in seg.items():
        d = n - seg.get((q, p), 0)
        if d > 0:
            out[(p, q)] = d
    return out


def shoelace_ids(ids, w1):
    xy = [(t % w1, t // w1) for t in ids]
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(xy, xy[1:] + xy[:1]))


def frame_cycle(loops_out, vertices_out):
    """the unpaired segments as one simple closed cycle of vertex ids; asserts that they are one, each with N = 1"""
    odd = unpaired(loops_out, vertices_out)
    if not odd:  # the frame itself came down to two vertices: a cycle whose two segments cancel
        return []
    assert all(n == 1 for n in odd.values())
    nxt = dict(odd.keys())
    assert len(nxt) == len(odd) and sorted(nxt) == sorted(nxt.values())  # every vertex is left once and entered once: simple
    first = min(nxt)
    cycle, p = [first], nxt[first]
    while p != first:
        cycle.append(p)
        p = nxt[p]
    assert len(cycle) == len(odd)  # one cycle
    return cycle


def check_invariants(plane, loops_out, vertices_out, counts_out, ringed=False):
    """nothing skipped: all segments pair up except one simple cycle, the frame, and the shoelace sums agree"""
    h, w = np.asarray(plane).shape
    assert counts_out[3] == 0 and len(loops_out) == counts_out[0] and len(vertices_out) == counts_out[1]
    cnt = loops_out[:, COUNT].astype(np.int64)
    assert (loops_out[:, OFFSET] == np.cumsum(cnt) - cnt).all() and int(cnt.sum()) == len(vertices_out)
    assert int(counts_out[2]) == int((cnt < 3).sum())
    cycle = frame_cycle(loops_out, vertices_out)
    v = np.asarray(vertices_out).tolist()
    total = sum(shoelace_ids(v[off:off + c], w + 1) for off, c, _, _ in loops_out.tolist())
    assert total == shoelace_ids(cycle, w + 1)
    if ringed:
        assert len(cycle) == 4 and total == 2 * h * w
    return cycle


def ring_holds(shape, tol16):
    """the tolerance below which a ringed plane's frame stays its four edges: tol16 / 16 < h * w / sqrt(h^2 + w^2)"""
    h, w = shape
    return tol16 * tol16 * (h * h + w * w) < 256 * h * h * w * w


def ring_around(plane, value):
    """the plane inside a one-pixel ring of `value`"""
    plane = np.asarray(plane)
    out = np.full((plane.shape[0] + 2, plane.shape[1] + 2), value, plane.dtype)
    out[1:-1, 1:-1] = plane
    return out


def bar_over_stripes(w, dtype=np.uint8):
    """row 0 one value, row 1 vertical stripes one pixel wide, all different from the bar and from their neighbours: the bar's lower
    edge is one straight edge with w - 1 junctions inside"""
    p = np.zeros((2, w), dtype)
    p[0] = 7
    p[1] = np.arange(w) % 3
    return p


# ---------------------------------------------------------------- the planes of the tests
def tee(k):
    """a 3 x 3 T: a bar over two halves, turned k times"""
    return np.ascontiguousarray(np.rot90(np.array([[1, 1, 1], [2, 2, 3], [2, 2, 3]], np.uint8), k))


@functools.lru_cache(maxsize=None)
def planes():
    """[(name, plane, skip value or None, ringed)]: computed once, shared, never changed"""
    u8, u32 = np.uint8, np.uint32
    out = [("1x1", np.array([[5]], u8), None, False), ("1x7", (np.arange(7, dtype=u8) // 2 % 2)[None, :].copy(), None, False),
           ("7x1", (np.arange(7, dtype=u8) // 3)[:, None].copy(), None, False),
           ("saddle", np.array([[1, 2], [2, 1]], u8), None, False), ("saddle with a none", np.array([[1, 2], [2, 9]], u8), 9, False),
           ("four values", np.array([[1, 2], [3, 4]], u8), None, False)]
    out += [(f"tee {k}", tee(k), None, False) for k in range(4)]
    for w in WIDTHS:
        bar = bar_over_stripes(w)
        out += [(f"bar {w}", bar, None, False), (f"bar {w} transposed", np.ascontiguousarray(bar.T), None, False),
                (f"bar {w} ringed", ring_around(bar, 9), None, True), (f"bar {w} transposed ringed", ring_around(np.ascontiguousarray(bar.T), 9), None, True)]
    noise = R.noise(24, 40, 5, seed=3)
    smooth = R.smooth(135, 240, seed=750)
    out += [("checkerboard", R.checkerboard(9, 11), None, False), ("noise", noise, None, False),
            ("noise ringed", ring_around(R.noise(17, 70, 2, seed=4), 9), None, True), ("staircase", R.staircase(40, 40), None, False),
            ("spiral", R.spiral(33, 47), None, False), ("serpentine", R.serpentine(20, 31), None, False), ("smooth", smooth, None, False)]
    # variants: u32 planes with 0xFFFFFFFF as a value, SKIP with a present and an absent value, a Regions label plane
    wide = noise.astype(u32)
    wide[wide == 0] = NONE_VALUE
    out += [("noise u32", wide, None, False), ("noise u32 skip 0xFFFFFFFF", wide, NONE_VALUE, False), ("noise skip present", noise, 2, False),
            ("noise skip absent", noise, 200, False), ("spiral u32", R.spiral(33, 47).astype(u32), None, False),
            ("staircase skip present", R.staircase(40, 40), int(R.staircase(40, 40)[0, 0]), False)]
    labels, _, _ = R.label(R.smooth(65, 130), None, 8, 6, R.SKIP_BACKGROUND)
    out.append(("labels", labels.astype(u32), NONE_VALUE, False))
    return out
