"""Reference of Tracks (region identities carried from frame to frame) for the tests: numpy only, no product code.

Semantics (include/infur_hip.h), applied literally:

* a step takes the Regions outputs of a frame (labels, table, n); regions with id < T = min(n, table_rows, max_regions) are
  tracked, the others get ``NONE`` and the status bit ``TRUNCATED``;
* ``overlap(c, p)`` counts the pixels whose current label c and remembered label p are both tracked -- ``np.unique`` over
  ``(c << 32) | p``; a pair is a candidate iff the classes agree and ``overlap >= max(min_overlap, 1)``;
* each c chooses its candidate of largest overlap (ties: smaller p); each p is kept by its chooser of largest overlap (ties:
  smaller c); a kept c inherits id and birth frame, ``AGE = age(p) + 1``; every other tracked c is new, ``AGE = 1``;
* new ids are ``next_id + rank`` in ascending region id; ``next_id + new > 0xFFFFFFFE`` is ``IDS_EXHAUSTED``: every region
  ``NONE``, ``next_id`` unchanged, the frame forgotten;
* first frame, reset, exhausted step before, or another h x w: everything new, ``ENDED = 0``;
* R = runs of equal tracked (c, p) along rows cut every 64 columns; ``2 R > pair_slots`` is ``OVERFLOW``: everything new,
  the frame is still remembered.

The sequence generators the CPU and GPU tests share are at the bottom; they build on ``regions_ref``'s planes.
"""
import numpy as np

import regions_ref as R

NONE = 0xFFFFFFFF
ID, AGE, BORN, PREV_REGION, OVERLAP, PREV_PIXELS, PREV_SUM_X, PREV_SUM_Y, WORDS = range(9)
TRUNCATED, OVERFLOW, IDS_EXHAUSTED = 1, 2, 4
STATUS, CONTINUED, NEW, ENDED = range(4)
DEFAULT_REGIONS, DEFAULT_SLOTS = 65536, 1 << 20


class Step:
    """one step's outputs: track_of_region [min(n, rows)] u32, table [min(n, rows), 8] u64, plane [h, w] u32, summary [4] u32;
    runs = R of the overflow rule"""

    def __init__(self, tor, table, plane, summary, runs):
        self.track_of_region, self.table, self.plane, self.summary, self.runs = tor, table, plane, summary, runs


class Tracker:
    def __init__(self, max_regions=0, pair_slots=0):
        self.M = max_regions or DEFAULT_REGIONS
        self.S = pair_slots or DEFAULT_SLOTS
        assert self.S >= 64 and self.S & (self.S - 1) == 0
        self.next_id = 0
        self.frame = 0
        self.valid = False

    def reset(self, first_id=0):
        self.valid = False
        self.next_id = first_id

    def step(self, labels, table, n, table_rows=None, min_overlap=1):
        labels = np.asarray(labels, np.uint32)
        h, w = labels.shape
        if h * w == 0:
            self.valid = False
            self.frame += 1
            return Step(np.zeros(0, np.uint32), np.zeros((0, WORDS), np.uint64), labels.copy(), np.zeros(4, np.uint32), 0)
        table = np.asarray(table, np.uint64).reshape(-1, R.WORDS)
        rows = len(table) if table_rows is None else table_rows
        nrows = min(n, rows)
        T = min(nrows, self.M)
        fresh = not (self.valid and (self.ph, self.pw) == (h, w))
        runs, pairs = 0, {}
        if not fresh:
            c, p = labels.astype(np.uint64), self.prev.astype(np.uint64)
            ok = (c < T) & (p < self.pT)
            key = np.where(ok, (c << np.uint64(32)) | p, np.uint64(0xFFFFFFFFFFFFFFFF))
            start = np.ones((h, w), bool)
            start[:, 1:] = key[:, 1:] != key[:, :-1]
            start[:, 64::64] = True
            runs = int((start & ok).sum())
        overflow = 2 * runs > self.S
        if not fresh and not overflow:
            keys, counts = np.unique(key[ok], return_counts=True)
            pairs = {(int(k) >> 32, int(k) & 0xFFFFFFFF): int(v) for k, v in zip(keys, counts)}
            assert len(pairs) <= runs
        klass = table[:, R.CLASS]
        best = {}  # c -> (overlap, p)
        for (c, p), ov in pairs.items():
            if int(klass[c]) == self.pclass[p] and ov >= max(min_overlap, 1):
                if c not in best or (ov, -p) > (best[c][0], -best[c][1]):
                    best[c] = (ov, p)
        claim = {}  # p -> (overlap, c)
        for c, (ov, p) in best.items():
            if p not in claim or (ov, -c) > (claim[p][0], -claim[p][1]):
                claim[p] = (ov, c)
        kept = {c: (ov, p) for c, (ov, p) in best.items() if claim[p][1] == c}
        new = T - len(kept)
        exhausted = self.next_id + new > 0xFFFFFFFE
        remembered = 0 if fresh else self.pT
        status = (TRUNCATED if T < n else 0) | (OVERFLOW if overflow else 0) | (IDS_EXHAUSTED if exhausted else 0)
        tt = np.zeros((nrows, WORDS), np.uint64)
        tt[:, ID] = NONE
        tt[:, PREV_REGION] = NONE
        track, age, born = [NONE] * T, [0] * T, [0] * T
        if not exhausted:
            rank = 0
            for c in range(T):
                if c in kept:
                    ov, p = kept[c]
                    track[c], age[c], born[c] = self.ptrack[p], self.page[p] + 1, self.pborn[p]
                    tt[c, PREV_REGION:] = (p, ov, self.ppix[p], self.psx[p], self.psy[p])
                else:
                    track[c], age[c], born[c] = self.next_id + rank, 1, self.frame
                    rank += 1
                tt[c, ID], tt[c, AGE], tt[c, BORN] = track[c], age[c], born[c]
            self.next_id += new
            summary = (status, T - new, new, remembered - (T - new))
        else:
            summary = (status, 0, 0, remembered)
        lut = np.full(T + 1, NONE, np.uint32)
        lut[:T] = track
        plane = lut[np.minimum(labels, T)]
        # what the next step sees of this frame
        self.valid = not exhausted
        self.ph, self.pw, self.pT, self.prev = h, w, T, labels.copy()
        self.pclass = [int(v) for v in klass[:T]]
        self.ppix, self.psx, self.psy = ([int(v) for v in table[:T, col]] for col in (R.PIXELS, R.SUM_X, R.SUM_Y))
        self.ptrack, self.page, self.pborn = track, age, born
        self.frame += 1
        return Step(tt[:, ID].astype(np.uint32), tt, plane, np.array(summary, np.uint32), runs)


def regions_of(klass, connectivity=R.CONNECT_8, min_pixels=0, flags=0):
    """class plane -> (labels, table, n): what a step takes"""
    return R.label(klass, R.conf_for(klass) if klass.size else None, connectivity, min_pixels, flags)


# ---------------------------------------------------------------- sequences of class planes
def identical(h, w):
    return [R.smooth(h, w)] * 3


def shift(h, w):
    k = R.smooth(h, w)
    return [np.roll(k, (i, 2 * i), axis=(0, 1)) for i in range(4)]


def _bar(h, w):
    """a horizontal bar of class 1 on class 0 that touches no border (where the plane has room for that)"""
    k = np.zeros((h, w), np.uint8)
    y0, y1 = (h // 4, max(h // 4 + 1, h // 2)) if h > 2 else (0, h)
    x0, x1 = (1, w - 1) if w > 2 else (0, w)
    k[y0:y1, x0:x1] = 1
    return k, (y0, y1, x0, x1)


def split(h, w, equal=False):
    """whole bar, then the bar cut by a one-pixel column of class 2 into a smaller left and a larger right part (equal: two
    parts of the same size; the bar's length is made odd for it)"""
    k, (y0, y1, x0, x1) = _bar(h, w)
    if equal and (x1 - x0) % 2 == 0:
        k[:, x1 - 1] = 0
        x1 -= 1
    cut = k.copy()
    cut[y0:y1, (x0 + x1) // 2 if equal else x0 + (x1 - x0) // 3] = 2
    return [k, cut]


def merge(h, w, equal=False):
    return split(h, w, equal)[::-1]


def class_change(h, w):
    k, _ = _bar(h, w)
    k2 = k.copy()
    k2[k == 1] = 2
    return [k, k2, k2]


def gap(h, w):
    k, _ = _bar(h, w)
    return [k, np.zeros_like(k), k]


def cross(h, w):
    return [R.stripes(h, w, True), R.stripes(h, w, False)]


def noise3(h, w):
    return [R.noise(h, w, 3, seed=s) for s in (0, 1, 2)]


def resize(h, w):
    a, b = R.smooth(h, w), R.smooth(h + 3, max(1, w - 5), seed=1)
    return [a, a, b, b, a]


FAMILIES = {"identical": identical, "shift": shift, "split": split, "split_equal": lambda h, w: split(h, w, True), "merge": merge,
            "merge_equal": lambda h, w: merge(h, w, True), "class_change": class_change, "gap": gap, "cross": cross, "noise3": noise3,
            "resize": resize}


def run(frames, tracker=None, table_rows=None, min_overlap=1, connectivity=R.CONNECT_8):
    """class planes through Regions' and this reference -> [(labels, table, n, Step)]"""
    tracker = tracker or Tracker()
    out = []
    for k in frames:
        labels, table, n = regions_of(k, connectivity)
        out.append((labels, table, n, tracker.step(labels, table, n, table_rows, min_overlap)))
    return out
