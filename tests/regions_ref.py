"""Reference of Regions (connected components of a class plane) for the tests: numpy / scipy only, no product code.

Semantics (include/infur_hip.h):

* a region is a maximal set of pixels of equal class, connected under 4- or 8-connectivity;
* ``flags & SKIP_BACKGROUND``: class-0 pixels form no region; ``min_pixels``: smaller regions are dropped; the pixels of
  either are labelled ``NONE``;
* kept regions are numbered densely from 0 in ascending order of FIRST, the smallest linear index ``y * w + x`` of the region;
* a table row is the eight Segments statistics words restricted to the region, then CLASS and FIRST.

``label`` is implemented twice: with ``scipy.ndimage.label`` class by class (when scipy imports) and as a run-based two-pass
union-find in numpy / Python that is always available.  Both hand an arbitrary partition numbering to ``canonical``, which
numbers by FIRST exactly as above.  The families of inputs the CPU and GPU tests share are at the bottom.
"""
import numpy as np

try:
    from scipy import ndimage as _ndi
    HAVE_SCIPY = True
except ImportError:  # a box without scipy still runs the suite on the numpy implementation
    _ndi = None
    HAVE_SCIPY = False

CONNECT_4, CONNECT_8 = 4, 8
SKIP_BACKGROUND = 1
PIXELS, SUM_X, SUM_Y, SUM_CONF, MIN_X, MIN_Y, MAX_X, MAX_Y, CLASS, FIRST, WORDS = range(11)
NONE = np.uint32(0xFFFFFFFF)
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def canonical(part, klass, conf, min_pixels, flags):
    """partition ids [h, w] (any integers, equal within a region and nowhere else) -> (labels u32 [h, w], table u64 [n, 10], n)"""
    h, w = klass.shape
    if h * w == 0:
        return np.zeros((h, w), np.uint32), np.zeros((0, WORDS), np.uint64), 0
    _, first, inverse, counts = np.unique(part.ravel(), return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.ravel()
    kflat = klass.ravel()
    keep = counts >= min_pixels
    if flags & SKIP_BACKGROUND:
        keep &= kflat[first] != 0
    kept = np.flatnonzero(keep)
    kept = kept[np.argsort(first[kept], kind="stable")]
    n = len(kept)
    new_id = np.full(len(first), int(NONE), np.int64)
    new_id[kept] = np.arange(n)
    lab = new_id[inverse]
    labels = lab.astype(np.uint32).reshape(h, w)
    table = np.zeros((n, WORDS), np.uint64)
    if n:
        m = lab != int(NONE)
        ids = lab[m]
        ys, xs = np.divmod(np.flatnonzero(m), w)
        cf = (conf.ravel()[m] if conf is not None else np.zeros(len(ids), np.uint8)).astype(np.float64)
        table[:, PIXELS] = np.bincount(ids, minlength=n).astype(np.uint64)
        for col, wt in ((SUM_X, xs), (SUM_Y, ys), (SUM_CONF, cf)):
            table[:, col] = np.round(np.bincount(ids, weights=wt.astype(np.float64), minlength=n)).astype(np.uint64)  # < 2^53: exact
        for col, v, fn, init in ((MIN_X, xs, np.minimum, h * w), (MIN_Y, ys, np.minimum, h * w), (MAX_X, xs, np.maximum, 0),
                                 (MAX_Y, ys, np.maximum, 0)):
            acc = np.full(n, init, np.int64)
            fn.at(acc, ids, v)
            table[:, col] = acc.astype(np.uint64)
        table[:, CLASS] = kflat[first[kept]].astype(np.uint64)
        table[:, FIRST] = first[kept].astype(np.uint64)
    return labels, table, n


def partition_scipy(klass, connectivity):
    structure = np.ones((3, 3), int) if connectivity == CONNECT_8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    part = np.zeros(klass.shape, np.int64)
    offset = 0
    for c in np.unique(klass):
        m = klass == c
        lab, k = _ndi.label(m, structure=structure)
        part[m] = lab[m].astype(np.int64) + offset
        offset += k
    return part


def partition_numpy(klass, connectivity):
    """two passes over horizontal runs: runs of equal class per row, then a union-find over the pairs of runs that touch"""
    h, w = klass.shape
    k = klass.astype(np.int32)
    start = np.ones((h, w), bool)
    start[:, 1:] = k[:, 1:] != k[:, :-1]
    run = (np.cumsum(start.ravel()) - 1).reshape(h, w)  # run ids in raster order
    pairs = []
    if h > 1:
        shifts = [(slice(None), slice(None))]
        if connectivity == CONNECT_8 and w > 1:
            shifts += [(slice(1, None), slice(None, -1)), (slice(None, -1), slice(1, None))]  # (below, above) column slices
        for below, above in shifts:
            same = k[1:, below] == k[:-1, above]
            pairs.append(np.stack([run[1:, below][same], run[:-1, above][same]], axis=1))
    parent = np.arange(int(run.max()) + 1)
    if pairs:
        uniq = np.unique(np.concatenate(pairs), axis=0)
        par = parent.tolist()
        for a, b in uniq.tolist():
            while par[a] != a:
                par[a] = par[par[a]]
                a = par[a]
            while par[b] != b:
                par[b] = par[par[b]]
                b = par[b]
            if a != b:
                if a < b:
                    par[b] = a
                else:
                    par[a] = b
        parent = np.asarray(par)
        while True:  # pointer jumping until every run points at its root
            nxt = parent[parent]
            if (nxt == parent).all():
                break
            parent = nxt
    return parent[run]


def label(klass, conf=None, connectivity=CONNECT_8, min_pixels=0, flags=0, impl=None):
    """-> (labels u32 [h, w], table u64 [n, 10], n);  impl: 'scipy', 'numpy' or None (scipy when it is there)"""
    assert connectivity in (CONNECT_4, CONNECT_8)
    klass = np.asarray(klass, np.uint8)
    if klass.size == 0:
        return canonical(None, klass, conf, min_pixels, flags)
    use_scipy = HAVE_SCIPY if impl is None else impl == "scipy"
    part = partition_scipy(klass, connectivity) if use_scipy else partition_numpy(klass, connectivity)
    return canonical(part, klass, conf, min_pixels, flags)


# ---------------------------------------------------------------- input families
def smooth(h, w, seed=0, classes=21, cell=24):
    """argmax of `classes` bilinearly up-sampled low-resolution Gaussian fields: blobs a few cells across, like a segmentation"""
    rng = np.random.default_rng(seed)
    lh, lw = h // cell + 2, w // cell + 2
    low = rng.normal(size=(classes, lh, lw))
    fy, fx = np.arange(h) / cell, np.arange(w) / cell
    y0, x0 = fy.astype(int), fx.astype(int)
    ty, tx = (fy - y0)[None, :, None], (fx - x0)[None, None, :]
    a = low[:, y0][:, :, x0]
    b = low[:, y0][:, :, x0 + 1]
    c = low[:, y0 + 1][:, :, x0]
    d = low[:, y0 + 1][:, :, x0 + 1]
    up = (a * (1 - tx) + b * tx) * (1 - ty) + (c * (1 - tx) + d * tx) * ty
    return up.argmax(axis=0).astype(np.uint8)


def noise(h, w, classes, seed=0):
    return np.random.default_rng(seed).integers(0, classes, size=(h, w), dtype=np.uint8)


def single(h, w, c=3):
    return np.full((h, w), c, np.uint8)


def serpentine(h, w):
    """one path, one pixel wide, running left to right and back on every second row: a single region that crosses every tile"""
    k = np.zeros((h, w), np.uint8)
    k[0::2] = 1
    for i, y in enumerate(range(1, h, 2)):
        k[y, (w - 1) if i % 2 == 0 else 0] = 1
    return k


def spiral(h, w, arms=1):
    """a rectangular spiral one pixel wide, walked inwards from the top-left corner with one pixel between its turns (class 1);
    what it leaves free is a second spiral: class 0, or class 2 with arms = 2"""
    k = np.zeros((h, w), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    k[0, 0] = 1
    while True:
        for _ in range(2):  # straight on while the pixel after the next is free, else one turn to the right
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not k[ny, nx] and not (0 <= ay < h and 0 <= ax < w and k[ay, ax]):
                break
            dy, dx = dx, -dy
        else:
            break
        y, x = ny, nx
        k[y, x] = 1
    if arms == 2:
        k[k == 0] = 2
    return k


def stripes(h, w, vertical=True):
    k = np.zeros((h, w), np.uint8)
    if vertical:
        k[:, 1::2] = 1
    else:
        k[1::2] = 1
    return k


def staircase(h, w, period=5):
    """diagonal lines one pixel wide: each is one region at connectivity 8 and as many regions as pixels at connectivity 4"""
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y) % period == 0).astype(np.uint8) * 7


def checkerboard(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y) & 1).astype(np.uint8)


def conf_for(klass, seed=1):
    return np.random.default_rng(seed).integers(0, 256, size=klass.shape, dtype=np.uint8)
