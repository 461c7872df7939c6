"""Reference of Anchors (a distance transform by value and one interior point per value) for the tests: numpy only, no product
code.

Semantics (include/infur_hip.h), applied literally:

* ``dist2[p]`` of a pixel p of value v is the squared Euclidean distance between pixel centres from p to the nearest position
  whose value differs from v; positions outside the frame count as differing, and so do skipped pixels for their neighbours;
* ``flags & SKIP``: pixels whose value equals ``skip_value`` belong to no region and read 0;
* row v < rows of the anchor table is (PIXEL = y*w + x of the pixel of value v with the largest dist2, ties to the smallest
  index; DIST2 = that dist2), or (NONE, 0) when no pixel that is not skipped holds v.

``distance`` is the separable form; ``distance_brute`` and ``distance_scipy`` restate the definition independently and exist only
to check it.
"""
import numpy as np

try:
    from scipy import ndimage

    HAVE_SCIPY = True
except ImportError:  # pragma: no cover
    HAVE_SCIPY = False

SKIP = 1
PIXEL, DIST2, WORDS = 0, 1, 2
NONE = 0xFFFFFFFF


def _kept(plane, flags, skip_value):
    return plane != plane.dtype.type(skip_value) if flags & SKIP else np.ones(plane.shape, bool)


def row_distance(plane):
    """g [h, w] int64: min(x - s + 1, e - x + 1) for the row run [s, e] of equal values around x"""
    h, w = plane.shape
    x = np.broadcast_to(np.arange(w, dtype=np.int64), (h, w))
    brk = np.ones((h, w), bool)
    brk[:, 1:] = plane[:, 1:] != plane[:, :-1]
    s = np.maximum.accumulate(np.where(brk, x, 0), axis=1)  # the last break at or before x
    end = np.ones((h, w), bool)
    end[:, :-1] = brk[:, 1:]
    e = np.minimum.accumulate(np.where(end, x, w)[:, ::-1], axis=1)[:, ::-1]  # the first end at or after x
    return np.minimum(x - s + 1, e - x + 1)


def distance(plane, flags=0, skip_value=0):
    """plane [h, w] of u8 or u32 -> dist2 u32 [h, w]"""
    plane = np.asarray(plane)
    assert plane.ndim == 2 and plane.dtype in (np.uint8, np.uint32)
    h, w = plane.shape
    if h * w == 0:
        return np.zeros((h, w), np.uint32)
    kept = _kept(plane, flags, skip_value)
    g = row_distance(plane)
    best = np.where(kept, g * g, 0)
    for sign in (-1, 1):  # up, then down: dy = 1, 2, .. while the column still holds the pixel's value
        alive = kept.copy()
        for dy in range(1, h + 1):
            alive &= dy * dy < best
            if not alive.any():
                break
            same = np.zeros((h, w), bool)  # (x, y + sign * dy) lies in the frame and holds the pixel's value
            f = np.zeros((h, w), np.int64)
            if dy < h:
                if sign < 0:
                    same[dy:] = plane[dy:] == plane[:-dy]
                    f[dy:] = g[:-dy]
                else:
                    same[:-dy] = plane[:-dy] == plane[dy:]
                    f[:-dy] = g[dy:]
            cand = dy * dy + np.where(same, f * f, 0)
            best = np.where(alive, np.minimum(best, cand), best)
            alive &= same
    return best.astype(np.uint32)


def distance_brute(plane, flags=0, skip_value=0):
    """the definition, pixel by pixel, over the plane padded by one ring of frame; for small shapes"""
    plane = np.asarray(plane)
    h, w = plane.shape
    pad = np.full((h + 2, w + 2), -1, np.int64)
    pad[1:-1, 1:-1] = plane
    qy, qx = np.mgrid[-1:h + 1, -1:w + 1]
    kept = _kept(plane, flags, skip_value)
    out = np.zeros((h, w), np.uint32)
    for y in range(h):
        for x in range(w):
            if kept[y, x]:
                d = (qy - y) ** 2 + (qx - x) ** 2
                out[y, x] = d[pad != int(plane[y, x])].min()
    return out


def distance_scipy(plane, flags=0, skip_value=0):
    """per value, scipy's exact Euclidean transform of the mask padded by one zero, squared and rounded"""
    plane = np.asarray(plane)
    h, w = plane.shape
    out = np.zeros((h, w), np.uint32)
    if h * w == 0:
        return out
    for v in np.unique(plane):
        if flags & SKIP and int(v) == skip_value:
            continue
        mask = np.zeros((h + 2, w + 2), bool)
        mask[1:-1, 1:-1] = plane == v
        d = ndimage.distance_transform_edt(mask)
        out[plane == v] = np.rint(d * d).astype(np.uint32)[1:-1, 1:-1][plane == v]
    return out


def anchors(plane, dist2, rows):
    """-> u32 [rows, 2]: per value v < rows the first pixel of the largest dist2 among those that hold v (a skipped pixel has
    dist2 0 and is none of them), (NONE, 0) where there is none"""
    out = np.zeros((rows, WORDS), np.uint32)
    out[:, PIXEL] = NONE
    value = np.asarray(plane).ravel().astype(np.int64)
    d = np.asarray(dist2).ravel().astype(np.int64)
    idx = np.flatnonzero((d > 0) & (value < rows))
    if len(idx) == 0:
        return out
    order = idx[np.lexsort((idx, -d[idx], value[idx]))]  # by value, then the largest distance, then the smallest index
    first = np.ones(len(order), bool)
    first[1:] = value[order][1:] != value[order][:-1]
    at = order[first]
    out[value[at], PIXEL] = at
    out[value[at], DIST2] = d[at]
    return out


# ---------------------------------------------------------------- input families regions_ref lacks
def disc(h, w, annulus=False):
    """class 1 within a circle about the plane's centre that leaves a margin (the nearest border is on no axis for most of
    its pixels); annulus: class 2 with a hole of class 0 of half the radius -- no pixel of the ring is at its centroid"""
    y, x = np.mgrid[0:h, 0:w]
    cy, cx, r = (h - 1) / 2.0, (w - 1) / 2.0, max(min(h, w) / 2.0 - 1.0, 0.5)
    d = (y - cy) ** 2 + (x - cx) ** 2
    k = (d <= r * r).astype(np.uint8)
    if annulus:
        k = k * 2
        k[d <= (r / 2) ** 2] = 0
    return k


def letter_c(h=24, w=24):
    """the square [2:h-2, 2:w-2] of class 1 with [7:h-7, 7:w-2] cut out of its right side: its centroid is a pixel of class 0"""
    k = np.zeros((h, w), np.uint8)
    k[2:h - 2, 2:w - 2] = 1
    k[7:h - 7, 7:w - 2] = 0
    return k
