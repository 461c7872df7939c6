"""Appearance's rule (include/infur_hip.h) in numpy: int64 sums per value by np.add.at, the histogram by np.bincount.  No product code."""
import numpy as np

SKIP = 1
WORDS, BINS = 12, 64
C_COUNTED, C_SKIPPED, C_OUTSIDE, C_VALUES, C_STATUS = 0, 1, 2, 3, 7
NOTHING = 1


def appearance(frame, plane, rows, flags=0, skip_value=0):
    """-> (table [rows, 12] u64, hist [rows, 64] u32, counts [8] u32)"""
    px = np.asarray(frame, np.uint8).reshape(-1, 3).astype(np.int64)
    v = np.asarray(plane).astype(np.int64).ravel()
    counted = v != skip_value if flags & SKIP else np.ones(v.shape, bool)
    inside = counted & (v < rows)
    v, px = v[inside], px[inside]
    b, g, r = px[:, 0], px[:, 1], px[:, 2]
    hist = np.bincount(v * BINS + ((r >> 6) << 4 | (g >> 6) << 2 | (b >> 6)), minlength=rows * BINS).reshape(rows, BINS)
    table = np.zeros((rows, WORDS), np.int64)
    for k, word in enumerate((np.ones_like(b), b, g, r, b * b, g * g, r * r, b * g, b * r, g * r)):
        np.add.at(table[:, k], v, word)
    if rows:
        table[:, 10] = hist.argmax(axis=1)  # (the first of equal maxima: the smallest bin)
        table[:, 11] = hist.max(axis=1)
    n = int(inside.sum())
    counts = [n, int((~counted).sum()), int(counted.sum()) - n, int((table[:, 0] > 0).sum()), 0, 0, 0, 0 if n else NOTHING]
    return table.astype(np.uint64), hist.astype(np.uint32), np.array(counts, np.uint32)
