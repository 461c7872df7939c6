"""Reference of Split (include/infur_hip.h) for the tests: numpy and plain Python only, no product code, sequential.

The rule, applied literally: pixels ordered by (height, -index); every kept pixel ascends to the largest larger 4-neighbour of its
value; basins named by their peaks; per pair of touching basins SADDLE and FIRST; Kruskal over the pairs in (SADDLE descending,
FIRST ascending) order, uniting when SADDLE >= core or when the two sets are not both marked; segments numbered by first pixel.
ROUNDS counts steps of the device's own construction of that forest and is not restated here: ``split`` leaves the word 0.
"""
import numpy as np

import anchors_ref

NONE = 0xFFFFFFFF
VALUE, PIXELS, FIRST, PEAK, HEIGHT, NECK, WORDS = range(7)
SEGMENTS, BASINS, PAIRS, RUNS, MARKED, SPLIT_VALUES, ROUNDS, STATUS, COUNT_WORDS = range(9)
OVERFLOW = 1


def dist2(plane, skip=None):  # Anchors' dist2 of the plane, from Anchors' own reference
    return anchors_ref.distance(plane, 1 if skip is not None else 0, skip or 0)


def basins(plane, height, skip=None):
    """-> (basin [h, w] int64: the peak index of every kept pixel, -1 on skipped ones)"""
    h, w = plane.shape
    n = h * w
    val, hgt = plane.ravel().astype(np.int64), height.ravel().astype(np.int64)
    kept = np.ones(n, bool) if skip is None else val != skip
    key = lambda i: (hgt[i], -i)  # noqa: E731
    up = np.arange(n)
    for i in range(n):
        if not kept[i]:
            continue
        y, x = divmod(i, w)
        nb = [j for j, ok in ((i - w, y > 0), (i - 1, x > 0), (i + 1, x + 1 < w), (i + w, y + 1 < h)) if ok and kept[j] and val[j] == val[i]]
        best = max(nb, key=key, default=i)
        if key(best) > key(i):
            up[i] = best
    out = np.full(n, -1, np.int64)
    for i in np.flatnonzero(kept):
        j = i
        while up[j] != j:
            j = up[j]
        out[i] = j
    return out.reshape(h, w)


def pairs_of(plane, basin, height):
    """-> ({(A, B): [SADDLE, FIRST]} with A < B, RUNS) over the edges between two kept pixels of one value and different basins"""
    h, w = basin.shape
    b, hg, val = basin.ravel(), height.ravel().astype(np.int64), plane.ravel().astype(np.int64)
    table, runs = {}, 0
    for i in range(h * w):
        y, x = divmod(i, w)
        for j, ok, edge, prev in ((i + 1, x + 1 < w, 2 * i, -w if y > 0 else None), (i + w, y + 1 < h, 2 * i + 1, -1 if x > 0 else None)):
            if not ok or b[i] < 0 or b[j] < 0 or b[i] == b[j] or val[i] != val[j]:
                continue
            rec = table.setdefault((min(b[i], b[j]), max(b[i], b[j])), [0, edge])
            rec[0] = max(rec[0], min(hg[i], hg[j]))
            # a run head: the edge one row up (towards x+1) or one column to the left (towards y+1) joins other basins
            if not (prev is not None and b[i + prev] == b[i] and b[j + prev] == b[j]):
                runs += 1
    return table, runs


class _Sets:
    def __init__(self):
        self.p = {}

    def find(self, a):
        self.p.setdefault(a, a)
        while self.p[a] != a:
            self.p[a] = a = self.p[self.p[a]]
        return a


def kruskal(table, peak_height, core):
    sets, marked = _Sets(), {b: hg >= core for b, hg in peak_height.items()}
    for (a, b), (saddle, _) in sorted(table.items(), key=lambda kv: (-kv[1][0], kv[1][1])):
        ra, rb = sets.find(a), sets.find(b)
        if ra != rb and (saddle >= core or not (marked[ra] and marked[rb])):
            sets.p[rb] = ra
            marked[ra] = marked[ra] or marked[rb]
    return {b: sets.find(b) for b in peak_height}


def split(plane, height, core, skip=None, rows=None, slots=1 << 20):
    """-> (labels [h, w] u32, table [min(n, rows), 6] u32, counts [8] u32); labels and table None when the pair table overflows"""
    h, w = plane.shape
    counts = np.zeros(COUNT_WORDS, np.uint32)
    if h * w == 0:
        return np.zeros((h, w), np.uint32), np.zeros((0, WORDS), np.uint32), counts
    basin = basins(plane, height, skip)
    val, b, hg = plane.ravel().astype(np.int64), basin.ravel(), height.ravel().astype(np.int64)
    table, runs = pairs_of(plane, basin, height)
    peaks = sorted(set(b[b >= 0].tolist()))
    counts[BASINS], counts[RUNS] = len(peaks), runs
    if 2 * runs > slots:
        counts[STATUS] = OVERFLOW
        return None, None, counts
    peak_height = {p: int(hg[p]) for p in peaks}
    root = kruskal(table, peak_height, core)
    labels = np.full(h * w, NONE, np.uint32)
    seg_of, recs = {}, []
    for i in range(h * w):
        if b[i] < 0:
            continue
        r = root[b[i]]
        if r not in seg_of:
            seg_of[r] = len(recs)
            recs.append([int(val[i]), 0, i, NONE, 0, 0])
        labels[i] = seg_of[r]
        recs[seg_of[r]][PIXELS] += 1
    for p in peaks:  # the largest peak of a segment in the order (height, -index)
        rec = recs[seg_of[root[p]]]
        if rec[PEAK] == NONE or (peak_height[p], -p) > (rec[HEIGHT], -rec[PEAK]):
            rec[PEAK], rec[HEIGHT] = p, peak_height[p]
    for (a, c), (saddle, _) in table.items():
        if root[a] != root[c]:
            for k in (a, c):
                rec = recs[seg_of[root[k]]]
                rec[NECK] = max(rec[NECK], saddle)
    values = [r[VALUE] for r in recs]
    counts[SEGMENTS], counts[PAIRS], counts[SPLIT_VALUES] = len(recs), len(table), sum(1 for v in set(values) if values.count(v) > 1)
    counts[MARKED] = sum(1 for p in peaks if peak_height[p] >= core)
    out = np.array(recs, np.uint32).reshape(-1, WORDS)
    return labels.reshape(h, w), out if rows is None else out[:rows], counts


# ---- the planes of the tests ----
def dumbbell(h=25, w=52, r=10, neck=2):
    c = h // 2
    y, x = np.mgrid[0:h, 0:w]
    m = ((y - c) ** 2 + (x - r - 2) ** 2 <= r * r) | ((y - c) ** 2 + (x - (w - r - 3)) ** 2 <= r * r) | ((abs(y - c) <= neck) & (x > r) & (x < w - r))
    return m.astype(np.uint8)


def bar():
    return np.pad(np.ones((7, 40), np.uint8), 2)


def band(h=24, w=50):
    y, x = np.mgrid[0:h, 0:w]
    return (abs(x - 2 * y) < 6).astype(np.uint8)
