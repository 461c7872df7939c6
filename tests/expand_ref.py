"""Reference of Expand (every open pixel takes the value of its exact nearest seed) for the tests: numpy only, no product code.

Semantics (include/infur_hip.h), applied literally, as a brute force: for each open pixel the minimum over ALL seeds of the
squared distance between pixel centres, ties to the smallest seed index y*w + x.  The open pixels are taken in chunks so that
a (135, 241) plane stays within seconds.
"""
import numpy as np

NONE = 0xFFFFFFFF
SEEDS, GAINED, MAX_D2, MAX_PIXEL, WORDS = 0, 1, 2, 3, 4
C_SEEDS, C_OPEN, C_GAINED, C_LEFT, C_MAX_D2, C_STATUS, C_WORDS = 0, 1, 2, 3, 4, 7, 8
NO_SEED = 1


def nearest(is_open, chunk=1 << 22):
    """is_open [h, w] bool -> (dist2, source), int64 [h * w]: 0 and the own index on a seed, NONE everywhere without any seed.
    This part of the answer depends on where the open pixels are and on nothing else."""
    h, w = is_open.shape
    seed, opn = np.flatnonzero(~is_open.ravel()), np.flatnonzero(is_open.ravel())  # ascending: argmin's first minimum is the tie rule
    if len(seed) == 0:
        return np.full(h * w, NONE, np.int64), np.full(h * w, NONE, np.int64)
    dist2, source = np.zeros(h * w, np.int64), np.arange(h * w, dtype=np.int64)
    sy, sx = (seed // w).astype(np.int32), (seed % w).astype(np.int32)  # (sides up to 32768: a sum of two squares stays below 2^31)
    step = max(1, chunk // len(seed))
    for i in range(0, len(opn), step):
        p = opn[i:i + step]
        dy, dx = (p // w).astype(np.int32)[:, None] - sy[None, :], (p % w).astype(np.int32)[:, None] - sx[None, :]
        d = dy * dy + dx * dx
        j = d.argmin(axis=1)
        dist2[p], source[p] = d[np.arange(len(p)), j], seed[j]
    return dist2, source


def expand(plane, open_value, reach=0, rows=0, near=None):
    """plane [h, w] of u8 or u32 -> (out like plane, dist2 u32 [h, w], source u32 [h, w], table u32 [rows, 4], counts u32 [8]);
    near: nearest(plane == open_value), where the caller has it already"""
    plane = np.asarray(plane)
    assert plane.ndim == 2 and plane.dtype in (np.uint8, np.uint32)
    h, w = plane.shape
    table = np.zeros((rows, WORDS), np.uint32)
    table[:, MAX_PIXEL] = NONE
    counts = np.zeros(C_WORDS, np.uint32)
    out = plane.copy()
    if h * w == 0:  # zero rows, zero counts and nothing else
        return out, np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32), table, counts
    is_open = plane == plane.dtype.type(open_value)
    dist2, source = near if near is not None else nearest(is_open)
    flat, opn = plane.ravel(), np.flatnonzero(is_open.ravel())
    counts[C_SEEDS], counts[C_OPEN] = h * w - len(opn), len(opn)
    if len(opn) == h * w:
        counts[C_LEFT], counts[C_STATUS] = len(opn), NO_SEED
    else:
        gained = opn[dist2[opn] <= reach * reach] if reach else opn
        res = out.ravel()
        res[gained] = flat[source[gained]]
        for v in range(rows):
            table[v, SEEDS] = int((flat[~is_open.ravel()] == v).sum())
            g = gained[res[gained] == v]  # ascending index: argmax's first maximum is the tie rule
            if len(g):
                table[v, GAINED], table[v, MAX_D2], table[v, MAX_PIXEL] = len(g), dist2[g].max(), g[dist2[g].argmax()]
        counts[C_GAINED], counts[C_LEFT] = len(gained), len(opn) - len(gained)
        counts[C_MAX_D2] = dist2[opn].max() if len(opn) else 0
    return out, dist2.astype(np.uint32).reshape(h, w), source.astype(np.uint32).reshape(h, w), table, counts
