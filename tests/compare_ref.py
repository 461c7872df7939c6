"""Reference of Compare (the confusion matrix and the best partner per value between two planes) for the tests: numpy only, no
product code.

Semantics (include/infur_hip.h), applied literally:

* two planes ``a`` and ``b`` of one h x w; a pixel with ``a == ignore_a`` (flag ``IGNORE_A``) or ``b == ignore_b`` (flag
  ``IGNORE_B``) is *ignored*, every other pixel is *compared*;
* a compared pixel with ``a >= rows_a`` or ``b >= rows_b`` is *outside*: counted, and part of nothing else; the rest are *inside*;
* ``matrix[i][j]`` counts the inside pixels with a == i and b == j;
* row i of ``rows_a``: PIXELS = the inside pixels of value i; PARTNER = the j of largest ``matrix[i][j]``, ties to the smallest
  j; INTER = that entry; UNION = PIXELS + the partner's PIXELS - INTER; ``(0, NONE, 0, 0)`` where PIXELS is 0.  ``rows_b`` is the
  mirror image.  A row is *matched* iff 2 INTER > UNION;
* ``counts`` = COMPARED, EQUAL (inside, a == b), IGNORED, OUTSIDE, PAIRS (non-zero entries), MATCHED (matched rows of a), RUNS,
  STATUS;
* RUNS = R = the runs of equal inside (i, j) along rows cut every 64 columns (Tracks' definition, tracks_ref.py);
* the form: ``rows_a * rows_b <= 4096`` is dense (STATUS 0, nothing can overflow); everything else goes through a pair table
  (STATUS has ``TABLE``) of ``pair_slots`` slots (0: 2^20), and ``2 R > pair_slots`` is ``OVERFLOW``: every PARTNER, INTER, UNION
  reads (NONE, 0, 0) and PAIRS = MATCHED = 0, while PIXELS, the matrix and the other counts stay exact;
* h * w == 0: zeros and NONE rows, STATUS 0.
"""
import numpy as np

NONE = 0xFFFFFFFF
IGNORE_A, IGNORE_B = 1, 2
PIXELS, PARTNER, INTER, UNION, WORDS = range(5)
COMPARED, EQUAL, IGNORED, OUTSIDE, PAIRS, MATCHED, RUNS, STATUS, COUNT_WORDS = range(9)
OVERFLOW, TABLE = 1, 2
DENSE_MAX, DEFAULT_SLOTS, MATRIX_MAX = 4096, 1 << 20, 1 << 20


class Result:
    """matrix [rows_a, rows_b] u32 (None above MATRIX_MAX entries), a [rows_a, 4] u32, b [rows_b, 4] u32, counts [8] u32"""

    def __init__(self, matrix, a, b, counts):
        self.matrix, self.a, self.b, self.counts = matrix, a, b, counts
        for arr in (matrix, a, b, counts):
            if arr is not None:
                arr.setflags(write=False)


def is_dense(rows_a, rows_b):
    return rows_a * rows_b <= DENSE_MAX


def classes_of(a, b, flags=0, ignore_a=0, ignore_b=0, rows_a=0, rows_b=0):
    """-> (ignored, outside, inside) boolean planes"""
    a, b = np.asarray(a).astype(np.uint64), np.asarray(b).astype(np.uint64)
    assert a.shape == b.shape and a.ndim == 2
    ignored = np.zeros(a.shape, bool)
    if flags & IGNORE_A:
        ignored |= a == ignore_a
    if flags & IGNORE_B:
        ignored |= b == ignore_b
    inside = ~ignored & (a < rows_a) & (b < rows_b)
    return ignored, ~ignored & ~inside, inside


def runs(a, b, inside):
    """R: the runs of equal inside (i, j) along rows cut every 64 columns"""
    h, w = inside.shape
    if h * w == 0:
        return 0
    key = np.where(inside, (np.asarray(a).astype(np.uint64) << np.uint64(32)) | np.asarray(b).astype(np.uint64), np.uint64(0xFFFFFFFFFFFFFFFF))
    start = np.ones((h, w), bool)
    start[:, 1:] = key[:, 1:] != key[:, :-1]
    start[:, 64::64] = True
    return int((start & inside).sum())


def _rows(pix, other_pix, pairs, side, overflow):
    """pairs: {(i, j): n}; side 0: the rows of a, 1: the rows of b"""
    out = np.zeros((len(pix), WORDS), np.uint32)
    out[:, PARTNER] = NONE
    out[:, PIXELS] = pix
    if overflow:
        return out
    best = {}
    for ij, n in pairs.items():
        me, partner = ij[side], ij[1 - side]
        if me not in best or (n, -partner) > (best[me][0], -best[me][1]):
            best[me] = (n, partner)
    for me, (n, partner) in best.items():
        out[me, PARTNER], out[me, INTER], out[me, UNION] = partner, n, int(pix[me]) + int(other_pix[partner]) - n
    return out


def compare(a, b, flags=0, ignore_a=0, ignore_b=0, rows_a=0, rows_b=0, pair_slots=0):
    a, b = np.asarray(a), np.asarray(b)
    ignored, outside, inside = classes_of(a, b, flags, ignore_a, ignore_b, rows_a, rows_b)
    small = rows_a * rows_b <= MATRIX_MAX
    counts = np.zeros(COUNT_WORDS, np.uint32)
    ia, ib = a[inside].astype(np.int64), b[inside].astype(np.int64)
    keys, n = np.unique((ia.astype(np.uint64) << np.uint64(32)) | ib.astype(np.uint64), return_counts=True)
    pairs = {(int(k) >> 32, int(k) & 0xFFFFFFFF): int(c) for k, c in zip(keys, n)}
    matrix = None
    if small:
        matrix = np.zeros((rows_a, rows_b), np.uint32)
        for (i, j), c in pairs.items():
            matrix[i, j] = c
    pix_a = np.bincount(ia, minlength=rows_a).astype(np.uint32) if rows_a else np.zeros(0, np.uint32)
    pix_b = np.bincount(ib, minlength=rows_b).astype(np.uint32) if rows_b else np.zeros(0, np.uint32)
    if a.size == 0:
        return Result(matrix, _rows(pix_a, pix_b, {}, 0, False), _rows(pix_b, pix_a, {}, 1, False), counts)
    R = runs(a, b, inside)
    table = not is_dense(rows_a, rows_b)
    overflow = table and 2 * R > (pair_slots or DEFAULT_SLOTS)
    ra, rb = _rows(pix_a, pix_b, pairs, 0, overflow), _rows(pix_b, pix_a, pairs, 1, overflow)
    counts[COMPARED] = int((~ignored).sum())
    counts[EQUAL] = int((ia == ib).sum())
    counts[IGNORED] = int(ignored.sum())
    counts[OUTSIDE] = int(outside.sum())
    counts[PAIRS] = 0 if overflow else len(pairs)
    counts[MATCHED] = int((2 * ra[:, INTER].astype(np.int64) > ra[:, UNION].astype(np.int64)).sum())
    counts[RUNS] = R
    counts[STATUS] = (TABLE if table else 0) | (OVERFLOW if overflow else 0)
    return Result(matrix, ra, rb, counts)


def brute(a, b, flags=0, ignore_a=0, ignore_b=0, rows_a=0, rows_b=0):
    """the definition as a double loop over the pixels, for tiny planes (the dense form's status; no overflow) -> Result"""
    a, b = np.asarray(a), np.asarray(b)
    h, w = a.shape
    matrix = np.zeros((rows_a, rows_b), np.uint32)
    counts = np.zeros(COUNT_WORDS, np.uint32)
    for y in range(h):
        prev = None
        for x in range(w):
            va, vb = int(a[y, x]), int(b[y, x])
            if ((flags & IGNORE_A) and va == ignore_a) or ((flags & IGNORE_B) and vb == ignore_b):
                counts[IGNORED] += 1
                prev = None
                continue
            counts[COMPARED] += 1
            if va >= rows_a or vb >= rows_b:
                counts[OUTSIDE] += 1
                prev = None
                continue
            matrix[va, vb] += 1
            counts[EQUAL] += va == vb
            if prev != (va, vb) or x % 64 == 0:
                counts[RUNS] += 1
            prev = (va, vb)
    rows = []
    for m in (matrix, matrix.T):
        out = np.zeros((m.shape[0], WORDS), np.uint32)
        for i in range(m.shape[0]):
            pix = int(m[i].sum())
            if not pix:
                out[i] = (0, NONE, 0, 0)
                continue
            j = max(range(m.shape[1]), key=lambda jj: (int(m[i, jj]), -jj))
            out[i] = (pix, j, m[i, j], pix + int(m[:, j].sum()) - int(m[i, j]))
        rows.append(out)
    counts[PAIRS] = int((matrix != 0).sum())
    counts[MATCHED] = sum(1 for r in rows[0] if 2 * int(r[INTER]) > int(r[UNION]))
    if not is_dense(rows_a, rows_b) and h * w:
        counts[STATUS] = TABLE
    return Result(matrix, rows[0], rows[1], counts)


def matched(rows):
    """the mask of matched rows of a row table"""
    rows = np.asarray(rows, np.int64)
    return 2 * rows[:, INTER] > rows[:, UNION]


# ---------------------------------------------------------------- input families
def shifted(plane, dy=1, dx=2):
    """the plane moved down and right, its own first rows and columns filling the gap: most pixels keep their class"""
    out = np.roll(np.roll(plane, dy, axis=0), dx, axis=1)
    out[:dy], out[:, :dx] = plane[:dy], plane[:, :dx]
    return out


WORKED_A = np.array([[0, 0, 1, 1], [0, 1, 1, 2]], np.uint8)
WORKED_B = np.array([[0, 0, 0, 1], [0, 1, 1, 1]], np.uint8)
