"""Reference of Outlines (region boundaries as closed polygon loops) for the tests: numpy and plain Python only, no product code.

A sequential tracer that applies the semantics of include/infur_hip.h literally:

* pixel p = (x, y), linear index i = y*w + x, sides N=0, E=1, S=2, W=3; side s of a kept pixel is an EDGE (id 4*i + s) when the
  neighbour across it is outside the plane, skipped (``flags & SKIP`` and value == ``skip_value``) or of another value;
* edges are directed with their pixel on the right hand: N heads east, E south, S west, W north -- the side is the heading d;
* the SUCCESSOR of an edge of value v that ends at vertex (X, Y), from the right-ahead pixel R and the left-ahead pixel L:
  both v -> turn left (L, d+3); only R -> straight (R, d); only L (the saddle) -> turn left under CONN8, else turn right
  (p, d+1); neither -> turn right (p, d+1).  The cycles of the successor are the LOOPS;
* a CORNER edge has another heading than its predecessor; a loop starts at its corner edge of the smallest id, loops are numbered
  in ascending order of that id, and a loop's vertices are the tail vertices (id Y*(w+1) + X) of its corner edges from the start on.
"""
import numpy as np

SKIP, CONN8 = 1, 2
OFFSET, COUNT, VALUE, START, WORDS = 0, 1, 2, 3, 4

_DX, _DY = (1, 0, -1, 0), (0, 1, 0, -1)  # one step along heading d = east, south, west, north
# head vertex of side d of pixel (x, y), as an offset from (x, y); the tail vertex of side d is the head of side d - 1
_HEAD = ((1, 0), (1, 1), (0, 1), (0, 0))
# the right-ahead and the left-ahead pixel of an edge that ends at vertex (X, Y) with heading d, as offsets from (X, Y)
_RIGHT = ((0, 0), (-1, 0), (-1, -1), (0, -1))
_LEFT = ((0, -1), (0, 0), (-1, 0), (-1, -1))


def padded(plane, flags=0, skip_value=0):
    """[h + 2, w + 2] int64: the plane with -1 around it and -1 at every skipped pixel, so that "is v" is ``== v``"""
    plane = np.asarray(plane)
    assert plane.ndim == 2 and plane.dtype in (np.uint8, np.uint32)
    h, w = plane.shape
    v = np.full((h + 2, w + 2), -1, np.int64)
    v[1:-1, 1:-1] = plane
    if flags & SKIP:
        v[1:-1, 1:-1][plane == skip_value] = -1
    return v


def edge_flags(plane, flags=0, skip_value=0):
    """-> bool [h, w, 4]: side s of pixel (x, y) is an edge"""
    v = padded(plane, flags, skip_value)
    c = v[1:-1, 1:-1]
    kept = c >= 0
    return np.stack([kept & (c != v[:-2, 1:-1]), kept & (c != v[1:-1, 2:]), kept & (c != v[2:, 1:-1]), kept & (c != v[1:-1, :-2])], axis=2)


def outline(plane, flags=0, skip_value=0, max_edges=0):
    """plane [h, w] of u8 or u32 -> (loops u32 [n_loops, 4], vertices u32 [n_vertices], counts u32 [3] = n_loops, n_vertices,
    n_edges).  max_edges: 0 = no limit; with more edges than that the result is (no loops, no vertices, {0, 0, n_edges})."""
    plane = np.asarray(plane)
    h, w = plane.shape
    assert 4 * h * w < 0xFFFFFFFF
    edge = edge_flags(plane, flags, skip_value).reshape(-1)
    n_edges = int(edge.sum())
    none = (np.zeros((0, WORDS), np.uint32), np.zeros(0, np.uint32))
    if n_edges == 0 or (max_edges and n_edges > max_edges):
        return none + (np.array([0, 0, n_edges], np.uint32),)
    v = padded(plane, flags, skip_value).tolist()
    conn8 = bool(flags & CONN8)
    is_edge = edge.tolist()
    seen = [False] * len(is_edge)
    found = []  # (start edge id, value, [vertex ids])
    for first in np.flatnonzero(edge).tolist():
        if seen[first]:
            continue
        cycle, e = [], first
        while not seen[e]:
            seen[e] = True
            cycle.append(e)
            i, d = e >> 2, e & 3
            x, y = i % w, i // w
            val = v[y + 1][x + 1]
            X, Y = x + _HEAD[d][0], y + _HEAD[d][1]
            rx, ry = X + _RIGHT[d][0], Y + _RIGHT[d][1]
            lx, ly = X + _LEFT[d][0], Y + _LEFT[d][1]
            r, l = v[ry + 1][rx + 1] == val, v[ly + 1][lx + 1] == val
            if l and (r or conn8):
                e = 4 * (ly * w + lx) + (d + 3) % 4
            elif r:
                e = 4 * (ry * w + rx) + d
            else:
                e = 4 * i + (d + 1) % 4
            assert is_edge[e], "the successor of an edge is an edge"
        assert e == first, "every edge has one predecessor: a walk closes where it began"
        corners = [c for k, c in enumerate(cycle) if (c & 3) != (cycle[k - 1] & 3)]
        at = corners.index(min(corners))
        corners = corners[at:] + corners[:at]
        verts = []
        for c in corners:
            i, d = c >> 2, c & 3
            tx, ty = _HEAD[(d + 3) % 4]
            verts.append((i // w + ty) * (w + 1) + i % w + tx)
        found.append((corners[0], v[(corners[0] >> 2) // w + 1][(corners[0] >> 2) % w + 1], verts))
    found.sort()
    loops = np.zeros((len(found), WORDS), np.uint32)
    at = 0
    for k, (start, val, verts) in enumerate(found):
        loops[k] = (at, len(verts), val, start)
        at += len(verts)
    vertices = np.array([t for f in found for t in f[2]], np.uint32)
    return loops, vertices, np.array([len(found), at, n_edges], np.uint32)


def polygons(loops, vertices, w):
    """-> [(value, is_hole, [(x, y), ...])] of complete loop records and their vertices"""
    out = []
    for off, cnt, val, start in np.asarray(loops).tolist():
        ids = np.asarray(vertices[off:off + cnt]).tolist()
        out.append((val, (start & 3) == 2, [(t % (w + 1), t // (w + 1)) for t in ids]))
    return out


def shoelace(xy):
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(xy, xy[1:] + xy[:1]))


def check_invariants(plane, flags, skip_value, loops, vertices, counts, first_of_label=None):
    """the facts that follow from the semantics.  first_of_label: the plane is a Regions label plane, and this maps a label to its
    region's first pixel -- the smallest START >> 2 among a region's outer loops is that pixel"""
    plane = np.asarray(plane)
    h, w = plane.shape
    kept = np.ones((h, w), bool) if not flags & SKIP else plane != skip_value
    loops, vertices = np.asarray(loops), np.asarray(vertices)
    assert loops.shape == (int(counts[0]), WORDS) and vertices.shape == (int(counts[1]),)
    assert int(counts[2]) == int(edge_flags(plane, flags, skip_value).sum())
    assert (loops[:, OFFSET] == np.cumsum(loops[:, COUNT]) - loops[:, COUNT]).all() and int(loops[:, COUNT].sum()) == len(vertices)
    assert (np.diff(loops[:, START].astype(np.int64)) > 0).all()
    total, outer_first = 0, {}
    for (val, hole, xy), (off, cnt, _, start) in zip(polygons(loops, vertices, w), loops.tolist()):
        assert cnt >= 4 and cnt % 2 == 0
        assert start & 3 in (0, 2) and hole == ((start & 3) == 2)
        assert int(plane.reshape(-1)[start >> 2]) == val and kept.reshape(-1)[start >> 2]
        assert all((x0 == x1) != (y0 == y1) for (x0, y0), (x1, y1) in zip(xy, xy[1:] + xy[:1]))  # axis-parallel, never zero-length
        assert all((xy[k - 1][0] == xy[k][0]) != (xy[k][0] == xy[(k + 1) % cnt][0]) for k in range(cnt))  # a turn at every vertex
        area2 = shoelace(xy)
        assert (area2 > 0) == (not hole) and area2 != 0
        total += area2
        if not hole:
            outer_first[val] = min(outer_first.get(val, start >> 2), start >> 2)
    assert total == 2 * int(kept.sum())
    if first_of_label is not None:
        assert outer_first == {int(k): int(f) for k, f in first_of_label.items()}


def snake(h, w):
    """one region of class 1 that winds through the whole plane: the even rows, joined at alternating ends, on class 0"""
    k = np.zeros((h, w), np.uint8)
    k[0::2] = 1
    for y in range(1, h, 2):
        k[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return k


def check_invariants_fast(plane, flags, skip_value, loops, vertices, counts):
    """the same facts in whole-array numpy, for planes with too many loops for the loop above (no per-vertex turn check)"""
    plane = np.asarray(plane)
    h, w = plane.shape
    kept = np.ones((h, w), bool) if not flags & SKIP else plane != skip_value
    loops, vertices = np.asarray(loops).astype(np.int64), np.asarray(vertices).astype(np.int64)
    assert loops.shape == (int(counts[0]), WORDS) and vertices.shape == (int(counts[1]),)
    assert int(counts[2]) == int(edge_flags(plane, flags, skip_value).sum())
    off, cnt, val, start = loops.T
    assert (off == np.cumsum(cnt) - cnt).all() and int(cnt.sum()) == len(vertices)
    assert (np.diff(start) > 0).all() and (cnt >= 4).all() and (cnt % 2 == 0).all() and np.isin(start & 3, (0, 2)).all()
    assert (plane.reshape(-1)[start >> 2] == val).all() and kept.reshape(-1)[start >> 2].all()
    x, y = vertices % (w + 1), vertices // (w + 1)
    assert (y <= h).all()
    nxt = np.arange(len(vertices)) + 1
    nxt[off + cnt - 1] = off
    assert ((x == x[nxt]) != (y == y[nxt])).all()
    area2 = np.add.reduceat(x * y[nxt] - x[nxt] * y, off) if len(off) else np.zeros(0, np.int64)
    assert ((area2 > 0) == ((start & 3) == 0)).all() and (area2 != 0).all()
    assert int(area2.sum()) == 2 * int(kept.sum())
