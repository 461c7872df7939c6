"""Reference of Tracks with memory (a gallery of lost tracks, include/infur_hip.h) for the tests: numpy only, no product code,
built on ``tracks_ref.Tracker``.  A step at frame counter f applies the eight phases of the header literally:

1. forget   a step that starts afresh (first frame, reset, set_memory, exhausted step before, another h x w) empties the
            gallery first; an empty frame (h * w = 0) empties it too and its memory summary is all zero
2. expire   gap(e) = f - SEEN(e) - 1; entries with gap > max_lost leave, EXPIRED counts them
3. match    Tracks' own match; the orphans are the tracked regions that no remembered region kept
4. candidates  (c, e): c an orphan, same class, box(c) intersects grow(box(e), reach * gap(e)) clamped to the plane;
            score = the intersection's area
5. revive   each orphan chooses its candidate of largest score (ties: smaller gallery index), each entry is kept by its
            chooser of largest score (ties: smaller c), a loser does not fall back
6. new ids  next_id + rank over the orphans that were not revived; exhaustion also empties the gallery
7. summary  NEW counts only new ids: CONTINUED + NEW + REVIVED = T
8. gallery  revived entries leave, the ended remembered regions are appended in ascending region id with SEEN = f - 1 (none
            on a step that started afresh), entries beyond gallery_rows are dropped from the front (GALLERY_FULL)

The vectorisation is over the gallery, per orphan.  The sequence generators of the memory tests are at the bottom.
"""
import numpy as np

import regions_ref as R
import tracks_ref as T

NONE = T.NONE
GALLERY_FULL = 8
L_ID, L_AGE, L_BORN, L_CLASS, L_PIXELS, L_SUM_X, L_SUM_Y, L_MIN_X, L_MIN_Y, L_MAX_X, L_MAX_Y, L_SEEN, L_WORDS = range(13)
REVIVED, LOST, EXPIRED, HELD = range(4)
DEFAULT_ROWS, MAX_ROWS = 4096, 65536


class MemStep(T.Step):
    """a step's outputs and what memory adds: gap_of_region [T] u32, memory [4] u32, gallery [HELD, 12] u64 (the gallery as the
    step left it); all three None on a tracker without memory"""

    def __init__(self, tor, table, plane, summary, runs, gap=None, memory=None, gallery=None):
        super().__init__(tor, table, plane, summary, runs)
        self.gap_of_region, self.memory, self.gallery = gap, memory, gallery


class Tracker(T.Tracker):
    def __init__(self, max_regions=0, pair_slots=0, max_lost=0, reach=0, gallery_rows=0):
        super().__init__(max_regions, pair_slots)
        self.set_memory(max_lost, reach, gallery_rows)

    def set_memory(self, max_lost, reach=0, gallery_rows=0):
        """forgets the remembered frame and the gallery; next_id and the frame counter keep counting"""
        self.max_lost, self.reach = max_lost, reach
        self.G = gallery_rows or DEFAULT_ROWS
        assert self.G <= MAX_ROWS or not max_lost  # (memory off: the other two arguments are ignored)
        self.valid = False
        self.gallery = np.zeros((0, L_WORDS), np.uint64)

    def reset(self, first_id=0):
        super().reset(first_id)
        self.gallery = np.zeros((0, L_WORDS), np.uint64)

    def _out(self, step, gap=None, memory=None):
        if not self.max_lost:
            return MemStep(step.track_of_region, step.table, step.plane, step.summary, step.runs)
        return MemStep(step.track_of_region, step.table, step.plane, step.summary, step.runs, np.asarray(gap, np.uint32),
                       np.asarray(memory, np.uint32), self.gallery.copy())

    def step(self, labels, table, n, table_rows=None, min_overlap=1):
        labels = np.asarray(labels, np.uint32)
        h, w = labels.shape
        if h * w == 0:
            self.gallery = self.gallery[:0]
            return self._out(super().step(labels, table, n, table_rows, min_overlap), np.zeros(0, np.uint32), np.zeros(4, np.uint32))
        table = np.asarray(table, np.uint64).reshape(-1, R.WORDS)
        rows = len(table) if table_rows is None else table_rows
        nrows = min(n, rows)
        Tn = min(nrows, self.M)
        f = self.frame
        fresh = not (self.valid and (self.ph, self.pw) == (h, w))
        # 1, 2: forget, expire
        gal, expired = self.gallery, 0
        if fresh or not self.max_lost:
            gal = gal[:0]
        gaps = f - gal[:, L_SEEN].astype(np.int64) - 1
        alive = gaps <= self.max_lost
        expired = int((~alive).sum())
        gal, gaps = gal[alive], gaps[alive]
        # 3: today's match
        runs, pairs = 0, {}
        if not fresh:
            c, p = labels.astype(np.uint64), self.prev.astype(np.uint64)
            ok = (c < Tn) & (p < self.pT)
            key = np.where(ok, (c << np.uint64(32)) | p, np.uint64(0xFFFFFFFFFFFFFFFF))
            start = np.ones((h, w), bool)
            start[:, 1:] = key[:, 1:] != key[:, :-1]
            start[:, 64::64] = True
            runs = int((start & ok).sum())
        overflow = 2 * runs > self.S
        if not fresh and not overflow:
            keys, counts = np.unique(key[ok], return_counts=True)
            pairs = {(int(k) >> 32, int(k) & 0xFFFFFFFF): int(v) for k, v in zip(keys, counts)}
        klass = table[:, R.CLASS]
        best = {}
        for (c, p), ov in pairs.items():
            if int(klass[c]) == self.pclass[p] and ov >= max(min_overlap, 1):
                if c not in best or (ov, -p) > (best[c][0], -best[c][1]):
                    best[c] = (ov, p)
        claim = {}
        for c, (ov, p) in best.items():
            if p not in claim or (ov, -c) > (claim[p][0], -claim[p][1]):
                claim[p] = (ov, c)
        kept = {c: (ov, p) for c, (ov, p) in best.items() if claim[p][1] == c}
        orphans = [c for c in range(Tn) if c not in kept]
        # 4, 5: candidates, revive
        rbest = {}  # c -> (score, e)
        if len(gal):
            grow = np.minimum(np.int64(self.reach) * gaps, np.int64(1) << 32)
            gx0 = np.maximum(gal[:, L_MIN_X].astype(np.int64) - grow, 0)
            gy0 = np.maximum(gal[:, L_MIN_Y].astype(np.int64) - grow, 0)
            gx1 = np.minimum(gal[:, L_MAX_X].astype(np.int64) + grow, w - 1)
            gy1 = np.minimum(gal[:, L_MAX_Y].astype(np.int64) + grow, h - 1)
            for c in orphans:
                x0, y0, x1, y1 = (int(table[c, col]) for col in (R.MIN_X, R.MIN_Y, R.MAX_X, R.MAX_Y))
                dx = np.minimum(gx1, x1) - np.maximum(gx0, x0) + 1
                dy = np.minimum(gy1, y1) - np.maximum(gy0, y0) + 1
                score = np.where((gal[:, L_CLASS] == klass[c]) & (dx > 0) & (dy > 0), dx * dy, 0)
                e = int(score.argmax())  # (the first of equal maxima: the smaller gallery index)
                if score[e] > 0:
                    rbest[c] = (int(score[e]), e)
        rclaim = {}
        for c, (sc, e) in rbest.items():
            if e not in rclaim or (sc, -c) > (rclaim[e][0], -rclaim[e][1]):
                rclaim[e] = (sc, c)
        revived = {c: e for c, (sc, e) in rbest.items() if rclaim[e][1] == c}
        # 6: new ids
        new = Tn - len(kept) - len(revived)
        exhausted = self.next_id + new > 0xFFFFFFFE
        remembered = 0 if fresh else self.pT
        status = (T.TRUNCATED if Tn < n else 0) | (T.OVERFLOW if overflow else 0) | (T.IDS_EXHAUSTED if exhausted else 0)
        tt = np.zeros((nrows, T.WORDS), np.uint64)
        tt[:, T.ID] = NONE
        tt[:, T.PREV_REGION] = NONE
        track, age, born, gap = [NONE] * Tn, [0] * Tn, [0] * Tn, [0] * Tn
        if not exhausted:
            rank = 0
            for c in range(Tn):
                if c in kept:
                    ov, p = kept[c]
                    track[c], age[c], born[c] = self.ptrack[p], self.page[p] + 1, self.pborn[p]
                    tt[c, T.PREV_REGION:] = (p, ov, self.ppix[p], self.psx[p], self.psy[p])
                elif c in revived:
                    e = gal[revived[c]]
                    track[c], age[c], born[c], gap[c] = int(e[L_ID]), int(e[L_AGE]) + 1, int(e[L_BORN]), int(gaps[revived[c]])
                    tt[c, T.PREV_PIXELS:] = (e[L_PIXELS], e[L_SUM_X], e[L_SUM_Y])
                else:
                    track[c], age[c], born[c] = self.next_id + rank, 1, self.frame
                    rank += 1
                tt[c, T.ID], tt[c, T.AGE], tt[c, T.BORN] = track[c], age[c], born[c]
            self.next_id += new
            # 7, 8: summary, gallery update
            ended = [p for p in range(remembered) if p not in claim]
            assert len(ended) == remembered - len(kept)
            lost = np.zeros((len(ended) if self.max_lost else 0, L_WORDS), np.uint64)
            for i, p in enumerate(ended[:len(lost)]):
                lost[i] = (self.ptrack[p], self.page[p], self.pborn[p], self.pclass[p], self.ppix[p], self.psx[p], self.psy[p], *self.pbox[p], f - 1)
            stay = np.ones(len(gal), bool)
            stay[list(revived.values())] = False
            gal = np.concatenate([gal[stay], lost])
            if len(gal) > self.G:
                gal = gal[len(gal) - self.G:]
                status |= GALLERY_FULL
            summary = (status, len(kept), new, remembered - len(kept))
            memory = (len(revived), len(lost), expired, len(gal))
        else:
            gal = gal[:0]
            summary = (status, 0, 0, remembered)
            memory = (0, 0, 0, 0)
        self.gallery = gal
        lut = np.full(Tn + 1, NONE, np.uint32)
        lut[:Tn] = track
        plane = lut[np.minimum(labels, Tn)]
        self.valid = not exhausted
        self.ph, self.pw, self.pT, self.prev = h, w, Tn, labels.copy()
        self.pclass = [int(v) for v in klass[:Tn]]
        self.ppix, self.psx, self.psy = ([int(v) for v in table[:Tn, col]] for col in (R.PIXELS, R.SUM_X, R.SUM_Y))
        self.pbox = [tuple(int(v) for v in table[c, R.MIN_X:R.MAX_Y + 1]) for c in range(Tn)]
        self.ptrack, self.page, self.pborn = track, age, born
        self.frame += 1
        return self._out(T.Step(tt[:, T.ID].astype(np.uint32), tt, plane, np.array(summary, np.uint32), runs), gap, memory)


def run(frames, tracker=None, table_rows=None, min_overlap=1, connectivity=R.CONNECT_8, **memory):
    """class planes through Regions' and this reference -> [(labels, table, n, MemStep)]"""
    tracker = tracker or Tracker(**memory)
    out = []
    for k in frames:
        labels, table, n = T.regions_of(k, connectivity)
        out.append((labels, table, n, tracker.step(labels, table, n, table_rows, min_overlap)))
    return out


# ---------------------------------------------------------------- sequences of class planes
def gap2(h, w):
    """bar, empty, empty, bar"""
    k, _ = T._bar(h, w)
    z = np.zeros_like(k)
    return [k, z, z, k]


def flicker(h, w):
    """class 1 reads as class 2 for one frame"""
    k = R.smooth(h, w)
    f = k.copy()
    f[k == 1] = 2
    return [k, f, k]


def flicker2(h, w):
    """flicker, then class 3 reads as class 0 for a frame, then two frames at rest"""
    k = R.smooth(h, w)
    g = k.copy()
    g[k == 3] = 0
    return flicker(h, w) + [g, k, k]


def drift(h, w):
    """bar, empty, and the bar h // 2 rows further down"""
    k, _ = T._bar(h, w)
    return [k, np.zeros_like(k), np.roll(k, h // 2, axis=0)]


def _squares(*boxes, h=33, w=96):
    """class planes of 8-high blocks on rows 8 .. 15: boxes = (x, width, class)"""
    k = np.zeros((h, w), np.uint8)
    for x, width, c in boxes:
        k[8:16, x:x + width] = c
    return k


def tie_two_to_one():
    return [_squares((8, 8, 1), (40, 8, 1)), _squares(), _squares((24, 8, 1))]


def tie_one_to_two():
    return [_squares((24, 8, 1)), _squares(), _squares((8, 8, 1), (40, 8, 1))]


def tie_larger_score():
    return [_squares((24, 8, 1)), _squares(), _squares((8, 8, 1), (38, 12, 1))]


def tie_other_class():
    return [_squares((24, 8, 1)), _squares(), _squares((24, 8, 2))]


TIES = {"two_to_one": tie_two_to_one, "one_to_two": tie_one_to_two, "larger_score": tie_larger_score, "other_class": tie_other_class}

FAMILIES = dict(T.FAMILIES, gap2=gap2, flicker=flicker, flicker2=flicker2, drift=drift)


def ragged4(ragged_scan_frames):
    """a, b, a, b of the two 96 x 128 planes of test_gpu_tracks.ragged_scan_frames() (Regions outputs, 4-connectivity)"""
    a, b = ragged_scan_frames
    return [a, b, a, b]


def ragged_scan_frames():
    """the same two planes as test_gpu_tracks.ragged_scan_frames(), built here so that a test without a GPU can use them"""
    a = R.noise(96, 128, 3, 0)
    b = a.copy()
    b[24:72] = R.noise(96, 128, 3, 100)[24:72]
    return tuple(T.regions_of(k, R.CONNECT_4) for k in (a, b))
